// The rules of closing many sessions in one pass (tree_close.hip) in plain
// C++, like zk_sess.h and zk_resume.h: the host compiler builds the very text
// the kernels run (tools/close_host.cpp puts it under ASan + UBSan on a
// machine without a GPU).  Three rules:
//   close_frame      which frames of a session batch close their segment
//   close_set_*      the set of closing session ids: open addressing over
//                    `cap` int64 keys (0 = empty) plus a parallel int32 rank,
//                    cap a power of two >= 2 K.  An id listed twice keeps the
//                    smallest list position; id 0 is never inserted and never
//                    found (eph[v] == 0 means "not ephemeral", so a listed 0
//                    removes nothing).  Every probe loop is bounded by cap,
//                    whatever the tables hold.
//   close_drop_mask  a listed watcher slot's bit in the drop mask
//
// The set's two writes go through an `Ops` policy: on the device a CAS on the
// key and an atomicMin on the rank (lanes insert concurrently), on the host
// their plain forms.  The rank table starts at CLOSE_NO_RANK everywhere (a
// byte fill of 0x7f), the key table at 0.
#pragma once
#include "zk_sess.h"

namespace zk {

// Does frame j (body [off, off + L) of rx[0, rx_len), segment seg) close its
// segment?  The table is sound, the segment is one of its S and its session
// alive (sess_refusal), the body holds an xid and an opcode, and the opcode is
// CLOSE_SESSION.  seg_state is read at an index in [0, S) only, rx inside
// [off, off + 8) only and only when the body lies inside rx.
ZK_HD bool close_frame(const uint8_t* __restrict__ rx, int64_t rx_len,
                       int64_t off, int64_t L,
                       const int64_t* __restrict__ bad,
                       const int32_t* __restrict__ seg_state, int64_t S,
                       int64_t seg) {
  if (sess_refusal(bad, seg_state, S, seg) != ERR_OK) return false;
  if (off < 0 || L < 8 || off > rx_len || L > rx_len - off) return false;
  return ld_be32(rx + off + 4) == OP_CLOSE_SESSION;
}

constexpr int32_t CLOSE_NO_RANK = 0x7f7f7f7f;

// The table size for K listed ids: the power of two >= 2 K (>= 2).
ZK_HD int64_t close_set_cap(int64_t K) {
  int64_t c = 2;
  while (c < 2 * K && c < ((int64_t)1 << 62)) c <<= 1;
  return c;
}

ZK_HD int64_t close_set_home(int64_t id, int64_t cap) {
  uint64_t x = (uint64_t)id;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (int64_t)(x & (uint64_t)(cap - 1));
}

// The plain forms of the set's two writes (one inserter at a time).
struct ClosePlainOps {
  // *p == expect ? (*p = want, expect) : *p
  ZK_HD int64_t cas(int64_t* p, int64_t expect, int64_t want) const {
    const int64_t old = *p;
    if (old == expect) *p = want;
    return old;
  }
  ZK_HD void amin(int32_t* p, int32_t v) const {
    if (v < *p) *p = v;
  }
};

// List position `pos` of id.  false: id 0 (not inserted), or no room in cap
// probes (a table of >= 2 K entries always has room for K ids).
template <class Ops>
ZK_HD bool close_set_insert(int64_t* __restrict__ key,
                            int32_t* __restrict__ rank, int64_t cap,
                            int64_t id, int32_t pos, const Ops& ops) {
  if (id == 0 || cap < 1) return false;
  int64_t s = close_set_home(id, cap);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const int64_t k = ops.cas(&key[s], 0, id);
    if (k == 0 || k == id) {
      ops.amin(&rank[s], pos);
      return true;
    }
    s = (s + 1) & (cap - 1);
  }
  return false;
}

// The smallest list position of id, or -1 when it is not in the set (after
// every insert is done: a later launch, or the same host thread).
ZK_HD int32_t close_set_find(const int64_t* __restrict__ key,
                             const int32_t* __restrict__ rank, int64_t cap,
                             int64_t id) {
  if (id == 0 || cap < 1) return -1;
  int64_t s = close_set_home(id, cap);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const int64_t k = key[s];
    if (k == 0) return -1;
    if (k == id) {
      const int32_t r = rank[s];
      return r >= 0 && r != CLOSE_NO_RANK ? r : -1;
    }
    s = (s + 1) & (cap - 1);
  }
  return -1;
}

// Watcher slot w's bit of the drop mask; a value outside 0..63 has none.
ZK_HD uint64_t close_drop_mask(int32_t w) {
  return w >= 0 && w < 64 ? (uint64_t)1 << w : 0;
}

}  // namespace zk
