// SET_ACL (opcode 7) in a session batch of any op mix
// (GpuServer.serve_sessions_mixed with setacl; the rule: zk_setacl.h).  The
// frames are of the ACL engine's class (zk_mix.h mix_class_setacl); the pass
// runs over the class's frame table before its GET_ACL frames are sized, so a
// GET_ACL of the batch sees the new ACL.  The launcher stands beside the ACL
// engine's (tree_acl.hip zk_tree_acl_setacl_sessions); here are the kernels:
//   setacl_judge_k   a lane per frame with opcode 7 of a served segment:
//                    setacl_frame, tree_lookup, and the ADMIN check on
//                    node_acl[node] as the pass finds it when the call carries
//                    the peers' addresses (the open ACL's word grants without
//                    a read of the arena, a lost binding denies).  A frame
//                    past every check but the version is pending; only those
//                    intern their vector — a client without ADMIN cannot fill
//                    the arena — by acl_intern_k's protocol (tree_acl.hip): one
//                    probe per distinct hash per wave, walked by the whole
//                    wave; an entry of an earlier launch is compared byte for
//                    byte while probing; the claimers take entry numbers and
//                    arena bytes with one atomic a wave each, copy and publish.
//   setacl_bind_k    the published word of the slot, the stored bytes compared
//                    with the frame's.  A vector that found no room fails its
//                    frame (SYSTEMERROR, counted) and leaves the node's ACL as
//                    it is.  A frame that later fails BAD_VERSION has interned
//                    its vector: nothing in this store is reclaimed.
//   setacl_claim_k / setacl_apply_k, `passes` rounds: every pending frame
//                    puts its index into its node's claim word with atomicMin
//                    (the deterministic leader, as list_mark_k claims parents);
//                    in the next launch the frame that finds its own index
//                    there checks its version against the slot's aversion
//                    (be32 at slot + 40), stores node_acl[node] and aversion + 1
//                    or takes BAD_VERSION, and puts the word back to idle.  The
//                    others stay pending.  So the SET_ACLs of a batch on one
//                    node take effect as a serial execution in frame order
//                    would, different nodes in parallel; a frame still pending
//                    after the rounds is answered SYSTEMERROR without effect
//                    and counted.
//   setacl_rows_k    the pass's frames into the ACL engine's rows (xid, err,
//                    slot, size: 4 + 84 bytes for a success, 4 + 16 for every
//                    failure), so the class's one scan sizes them with the
//                    GET_ACL replies, in request order; and the flags of the
//                    frames that reached the version check: each takes a zxid,
//                    failed ones included (the tree's rule, zk_tree.h), from a
//                    device-wide scan of the flags — unique, increasing in
//                    frame order, above every zxid of the serve's class (whose
//                    finish has run).
//   setacl_write_k   acl_write_k with a zxid and an aversion a frame: EIGHT
//                    lanes a reply, 16-byte pieces.  A success is header +
//                    the node's Stat from its slot with the aversion THIS frame
//                    produced (the slot holds the last one of the batch).
//   setacl_finish_k  the tree's zxid counter past the largest.
// No lane waits for another inside a launch; every grid comes from ncap;
// nothing is read back.  Every read of a frame is inside rx and the frame, of
// the tables inside ncap / S / the node capacity, of the arena inside
// arena_cap.
#include "zk_setacl_dev.h"
#include "zk_aclperm_dev.h"

namespace zk {

ZK_DEV int32_t setacl_row_count(const ZkAuthTable& au, int64_t seg) {
  if (!sess_in(seg, au.S)) return 0;
  const int32_t c = au.cnt[seg];
  return c < 0 ? 0 : (c < AUTH_K ? c : AUTH_K);
}

__global__ __launch_bounds__(TR_T) void setacl_judge_k(
    ZkTree t, ZkAclTable a, const uint8_t* __restrict__ rx, int64_t rx_len,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, SegTable M,
    const int32_t* __restrict__ addrs, ZkAuthTable au, SetAclWs w,
    int64_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int lane = lane_id();
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  int32_t state = SS_NONE, err = ERR_OK, xid = 0, ver = -1, len = 0;
  int64_t node = -1, nslot = -1, off = -1;
  bool denied = false, invalid = false;
  uint64_t h = 0;
  if (i < nf) {
    const int64_t seg = M.f_seg[i];
    const int64_t base = foff[i], L = flen[i];
    if (sess_refusal(M.bad, M.seg_state, M.S, seg) == ERR_OK && base >= 0 &&
        L >= 8 && base <= rx_len && L <= rx_len - base &&
        ld_be32(rx + base + 4) == OP_SET_ACL) {
      const SetAclFrame f = setacl_frame(rx, base, L);
      xid = f.xid;
      state = SS_FINAL;
      bool exists = false, admin = true;
      if (f.status == SF_OK) {
        const Found fd = tree_lookup(t, rx + f.poff, f.pl);
        exists = fd.node >= 0 && fd.node < a.cap && fd.node < t.store.cap;
        if (exists) {
          node = fd.node;
          nslot = fd.slot;
          if (addrs != nullptr) {
            const int64_t word = a.node_acl[node];
            const int32_t kind = !acl_word_ok(a, word) ? SA_LOST
                                 : acl_off(word) == 0 ? SA_OPEN : SA_VECTOR;
            const uint8_t* vec = a.arena + (kind == SA_VECTOR ? acl_off(word)
                                                              : 0);
            const uint8_t* ids = nullptr;
            int32_t nids = 0;
            if (au.recs != nullptr) {
              nids = setacl_row_count(au, seg);
              ids = au.recs + (nids > 0 ? seg * AUTH_ROW : 0);
            }
            admin = setacl_admin(kind, vec, acl_len(word), (uint32_t)addrs[seg],
                                 ids, nids);
          }
        }
      }
      // (the version is judged by the round that reaches the frame)
      err = setacl_verdict(f.status, exists, admin, -1, 0);
      denied = err == ERR_NO_AUTH;
      invalid = err == ERR_INVALID_ACL;
      if (err == ERR_OK) {
        if (nslot < 0 || nslot + STAT_BYTES > t.slab_cap) {
          err = ERR_SYSTEM;
        } else {
          state = SS_PEND;
          ver = f.version;
          off = f.voff;
          len = (int32_t)f.vlen;
          h = path_hash(rx + off, len) | 1ull;
        }
      }
    }
  }
  aclperm_count(&stats[SAS_DENIED], denied);
  aclperm_count(&stats[SAS_INVALID], invalid);
  // ---- the intern index: acl_intern_k's protocol (tree_acl.hip) ------------
  int32_t slot = AS_NONE;
  const bool need = state == SS_PEND;
  if (need) slot = AS_LOST;
  const int64_t old_top = a.ctr[AC_OLD_TOP];
  bool claimed = false;
  int64_t cslot = -1;
  uint64_t todo = __ballot(need);
  while (todo != 0) {
    const int first = __ffsll((unsigned long long)todo) - 1;
    const uint64_t h0 = __shfl(h, first, 64);
    const bool mine = need && h == h0;
    const uint64_t m = __ballot(mine);
    // (wave-uniform control flow: every value that decides a branch is the
    // leader's, broadcast; the leader alone claims)
    const int64_t loff = __shfl(off, first, 64);
    const int32_t llen = __shfl(len, first, 64);
    int64_t s = (int64_t)(h0 >> 8) & a.hmask;
    bool hit = false;
    for (int64_t probe = 0; probe <= a.hmask; ++probe) {
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
          // an earlier launch's entry: its bytes against the leader's
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
    w.state[i] = state;
    w.err[i] = err;
    w.xid[i] = xid;
    w.ver[i] = ver;
    w.vlen[i] = len;
    w.islot[i] = slot;
    w.aver[i] = 0;
    w.node[i] = node;
    w.nslot[i] = nslot;
    w.voff[i] = off;
    w.word[i] = ACL_LOST;
    w.zflag[i] = 0;
  }
}

__global__ __launch_bounds__(TR_T) void setacl_bind_k(
    ZkAclTable a, const uint8_t* __restrict__ rx, int64_t ncap, SetAclWs w,
    int64_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  // (nothing claims arena bytes in this launch: the top is this pass's)
  if (i == 0) a.ctr[AC_OLD_TOP] = a.ctr[AC_TOP];
  bool full = false;
  if (i < ncap && w.state[i] == SS_PEND) {
    const int32_t slot = w.islot[i];
    int64_t word = ACL_LOST;
    if (slot >= 0 && (int64_t)slot <= a.hmask) {
      const int64_t v = a.val[slot];
      const int32_t len = w.vlen[i];
      if (acl_word_ok(a, v) && acl_len(v) == len &&
          bytes_eq(a.arena + acl_off(v), rx + w.voff[i], len))
        word = v;
    }
    full = word == ACL_LOST;
    if (full) {
      w.state[i] = SS_FINAL;
      w.err[i] = ERR_SYSTEM;
    } else {
      w.word[i] = word;
    }
  }
  aclperm_count(&stats[SAS_STORE_FULL], full);
}

__global__ __launch_bounds__(TR_T) void setacl_claim_k(
    int64_t ncap, int64_t node_cap, SetAclWs w, int32_t* __restrict__ claim) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap || w.state[i] != SS_PEND) return;
  const int64_t node = w.node[i];
  if (node >= 0 && node < node_cap) atomicMin(&claim[node], (int32_t)i);
}

__global__ __launch_bounds__(TR_T) void setacl_apply_k(
    ZkTree t, ZkAclTable a, int64_t ncap, int64_t node_cap, SetAclWs w,
    int32_t* __restrict__ claim) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap || w.state[i] != SS_PEND) return;
  const int64_t node = w.node[i];
  if (node < 0 || node >= node_cap) return;
  if (__hip_atomic_load(&claim[node], __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT) != (int32_t)i)
    return;                                        // (a later round's)
  uint8_t* slot = t.store.slab + w.nslot[i];
  const int32_t av = ld_be32(slot + 40);
  const int32_t ver = w.ver[i];
  int32_t err = ERR_OK;
  if (ver != -1 && ver != av) {
    err = ERR_BAD_VERSION;
  } else {
    a.node_acl[node] = w.word[i];
    st_be32(slot + 40, av + 1);
    w.aver[i] = av + 1;
  }
  w.err[i] = err;
  w.state[i] = SS_FINAL;
  w.zflag[i] = 1;
  __hip_atomic_store(&claim[node], SETACL_IDLE, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TR_T) void setacl_rows_k(
    const int64_t* __restrict__ n_dev, int64_t ncap, SetAclWs w, SetAclRows r,
    int64_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  bool applied = false, badv = false, unreached = false;
  if (i < nf && w.state[i] != SS_NONE) {
    unreached = w.state[i] == SS_PEND;
    const int32_t err = unreached ? ERR_SYSTEM : w.err[i];
    applied = err == ERR_OK;
    badv = err == ERR_BAD_VERSION;
    r.xid[i] = w.xid[i];
    r.err[i] = err;
    r.word[i] = 0;                                 // (no vector in the reply)
    r.nslot[i] = applied ? w.nslot[i] : -1;
    r.sizes[i] = 4 + 16 + (applied ? STAT_BYTES : 0);
  }
  aclperm_count(&stats[SAS_APPLIED], applied);
  aclperm_count(&stats[SAS_BAD_VERSION], badv);
  aclperm_count(&stats[SAS_UNREACHED], unreached);
}

constexpr int SETACL_GROUP = 8;                    // lanes per reply
constexpr int64_t SETACL_HEAD = 4 + 16;
constexpr int64_t SETACL_AVER = 40;                // aversion in the Stat

__global__ __launch_bounds__(TR_T) void setacl_write_k(
    ZkTree t, ZkAclTable a, const int64_t* __restrict__ n_dev, int64_t ncap,
    SetAclWs w, SetAclRows r, const int64_t* __restrict__ rec_off,
    uint8_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t i = g / SETACL_GROUP;
  const int l = (int)(g % SETACL_GROUP);
  if (i >= ncap || i >= *n_dev || *r.over != 0) return;
  uint8_t* o = out + rec_off[i];
  const int64_t R = r.sizes[i];
  const int32_t err = r.err[i];
  const int64_t word = r.word[i];
  const int64_t A = err == ERR_OK ? (int64_t)acl_len(word) : 0;
  const uint8_t* ap = a.arena + (err == ERR_OK ? acl_off(word) : 0);
  const uint8_t* sp = t.store.slab + (err == ERR_OK ? r.nslot[i] : 0);
  // reads see the batch's base; a SET_ACL that reached its version check has
  // a zxid of its own
  const int64_t zx = t.counters[TC_ZXID] +
                     (w.zflag[i] != 0 ? w.zoff[i] + 1 : 0);
  const bool set = w.state[i] != SS_NONE && err == ERR_OK;
  const uint32_t aver = bswap32((uint32_t)w.aver[i]);
  const uint32_t head[5] = {
      bswap32((uint32_t)(R - 4)), bswap32((uint32_t)r.xid[i]),
      bswap32((uint32_t)((uint64_t)zx >> 32)), bswap32((uint32_t)zx),
      bswap32((uint32_t)err)};
  const int64_t seam = SETACL_HEAD + A;            // the Stat's first byte
  for (int64_t p = (int64_t)l * 16; p < R; p += SETACL_GROUP * 16) {
    if (p >= SETACL_HEAD && p + 16 <= seam) {
      uint4 x;
      __builtin_memcpy(&x, ap + (p - SETACL_HEAD), 16);
      __builtin_memcpy(o + p, &x, 16);
      continue;
    }
    if (p >= seam && p + 16 <= R) {
      uint4 x;
      __builtin_memcpy(&x, sp + (p - seam), 16);
      if (set) {
        // (the Stat of a SET_ACL reply starts at byte 20: the aversion is
        // one whole dword of one piece)
        const int64_t d = seam + SETACL_AVER - p;
        if (d == 0) x.x = aver;
        else if (d == 4) x.y = aver;
        else if (d == 8) x.z = aver;
        else if (d == 12) x.w = aver;
      }
      __builtin_memcpy(o + p, &x, 16);
      continue;
    }
    const int64_t pe = min(p + 16, R);
    for (int64_t q = p; q < pe; q += 4) {
      uint32_t x;
      if (q < SETACL_HEAD) {
        // (a select chain, not an indexed read: head[] stays in registers)
        const int k = (int)(q >> 2);
        x = k == 0 ? head[0] : k == 1 ? head[1] : k == 2 ? head[2]
            : k == 3 ? head[3] : head[4];
        __builtin_memcpy(o + q, &x, 4);
      } else if (q + 4 <= seam) {
        __builtin_memcpy(&x, ap + (q - SETACL_HEAD), 4);
        __builtin_memcpy(o + q, &x, 4);
      } else if (q >= seam && q + 4 <= R) {
        __builtin_memcpy(&x, sp + (q - seam), 4);
        if (set && q - seam == SETACL_AVER) x = aver;
        __builtin_memcpy(o + q, &x, 4);
      } else {
        const int64_t qe = min(q + 4, R);
        for (int64_t b = q; b < qe; ++b)
          o[b] = b < seam ? ap[b - SETACL_HEAD] : sp[b - seam];
      }
    }
  }
}

__global__ void setacl_finish_k(ZkTree t, SetAclWs w) {
  const int64_t n = w.ctr[0];
  if (n > 0) t.counters[TC_ZXID] += n;
}

// ---- the host functions the ACL engine's launcher calls ----------------------

int64_t setacl_layout(int64_t ncap, uint8_t* ws, SetAclWs* w) {
  auto a16 = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    uint8_t* p = ws != nullptr ? ws + o : nullptr;
    o += a16(bytes);
    return p;
  };
  uint8_t* ctr = take(64);
  uint8_t* i32s[7];
  for (auto& p : i32s) p = take(ncap * 4);
  uint8_t* i64s[6];
  for (auto& p : i64s) p = take(ncap * 8);
  uint8_t* scan = take(zk_scan_workspace(ncap > 0 ? ncap : 1) * 8);
  if (w != nullptr) {
    w->ctr = (int64_t*)ctr;
    w->state = (int32_t*)i32s[0];
    w->err = (int32_t*)i32s[1];
    w->xid = (int32_t*)i32s[2];
    w->ver = (int32_t*)i32s[3];
    w->vlen = (int32_t*)i32s[4];
    w->islot = (int32_t*)i32s[5];
    w->aver = (int32_t*)i32s[6];
    w->node = (int64_t*)i64s[0];
    w->nslot = (int64_t*)i64s[1];
    w->voff = (int64_t*)i64s[2];
    w->word = (int64_t*)i64s[3];
    w->zflag = (int64_t*)i64s[4];
    w->zoff = (int64_t*)i64s[5];
    w->scan = (int64_t*)scan;
  }
  return o;
}

int setacl_pass(const ZkTree& t, const ZkAclTable& a, const uint8_t* rx,
                int64_t rx_len, const int64_t* foff, const int32_t* flen,
                const int64_t* n_dev, int64_t ncap, const SegTable& M,
                const int32_t* addrs, const ZkAuthTable* au, int32_t passes,
                int32_t* claim, const SetAclWs& w, int64_t* stats,
                hipStream_t st) {
  const unsigned nb = (unsigned)((ncap + TR_T - 1) / TR_T);
  const ZkAuthTable none{nullptr, nullptr, nullptr, 0};
  const int64_t node_cap = a.cap < t.store.cap ? a.cap : t.store.cap;
  setacl_judge_k<<<nb, TR_T, 0, st>>>(t, a, rx, rx_len, foff, flen, n_dev,
                                      ncap, M, addrs,
                                      au != nullptr ? *au : none, w, stats);
  ZK_LAUNCH_CHECK();
  setacl_bind_k<<<nb, TR_T, 0, st>>>(a, rx, ncap, w, stats);
  ZK_LAUNCH_CHECK();
  for (int32_t p = 0; p < passes; ++p) {
    setacl_claim_k<<<nb, TR_T, 0, st>>>(ncap, node_cap, w, claim);
    ZK_LAUNCH_CHECK();
    setacl_apply_k<<<nb, TR_T, 0, st>>>(t, a, ncap, node_cap, w, claim);
    ZK_LAUNCH_CHECK();
  }
  return 0;
}

int setacl_rows(const int64_t* n_dev, int64_t ncap, const SetAclWs& w,
                const SetAclRows& r, int64_t* stats, hipStream_t st) {
  const unsigned nb = (unsigned)((ncap + TR_T - 1) / TR_T);
  setacl_rows_k<<<nb, TR_T, 0, st>>>(n_dev, ncap, w, r, stats);
  ZK_LAUNCH_CHECK();
  return zk_scan_excl_i64(w.zflag, w.zoff, ncap, &w.ctr[0], w.scan, st);
}

int setacl_write(const ZkTree& t, const ZkAclTable& a, const int64_t* n_dev,
                 int64_t ncap, const SetAclWs& w, const SetAclRows& r,
                 const int64_t* rec_off, uint8_t* out, hipStream_t st) {
  const unsigned nbw =
      (unsigned)((ncap * SETACL_GROUP + TR_T - 1) / TR_T);
  setacl_write_k<<<nbw, TR_T, 0, st>>>(t, a, n_dev, ncap, w, r, rec_off, out);
  ZK_LAUNCH_CHECK();
  setacl_finish_k<<<1, 1, 0, st>>>(t, w);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace zk

extern "C" {

// Bytes of the SET_ACL pass's workspace for up to ncap frames of the class
// (16-aligned parts).  Nothing in it needs zeroing.
int64_t zk_tree_setacl_workspace(int64_t ncap) {
  return zk::setacl_layout(ncap > 0 ? ncap : 0, nullptr, nullptr);
}

}  // extern "C"
