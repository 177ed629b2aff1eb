// The ACL store's words and counters (ZkAclTable, zk_abi.h), shared by the
// ACL path (tree_acl.hip) and the image load (tree_snap.hip), which binds
// the vectors of an image through the same index.
#pragma once
#include "zk_tree.h"

namespace zk {

// ACL_LOST: the store had no room for the vector (full index, full arena,
// the entry limit, or two new vectors of one batch with one hash); a GET_ACL
// on such a node answers SYSTEMERROR.  Nothing is ever reclaimed.
constexpr int64_t ACL_LOST = -1;
constexpr int64_t ACL_LEN_MAX = 1 << 24;
// ctr[]: arena top (a bump allocator: a claim that does not fit stays added,
// so the arena then counts as full), entries, nodes bound lost, the arena
// top when the last record pass ended, the entry limit (set by the owner)
enum : int { AC_TOP = 0, AC_ENT = 1, AC_LOST = 2, AC_OLD_TOP = 3,
             AC_LIMIT = 4 };
// per request of a record pass: the index slot its vector landed on
constexpr int32_t AS_NONE = -2;                // not a successful CREATE
constexpr int32_t AS_LOST = -1;                // no slot

ZK_DEV int64_t acl_off(int64_t w) { return w >> 24; }
ZK_DEV int32_t acl_len(int64_t w) { return (int32_t)(w & 0xFFFFFF); }
// a word that names bytes inside the arena (anything else reads as lost)
ZK_DEV bool acl_word_ok(const ZkAclTable& a, int64_t w) {
  return w > 0 && acl_len(w) >= 4 && acl_off(w) + acl_len(w) <= a.arena_cap;
}
ZK_DEV int64_t ld_relaxed(const int64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace zk
