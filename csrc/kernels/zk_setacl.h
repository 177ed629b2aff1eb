// The rule of SET_ACL (opcode 7) in plain C++, like zk_auth.h and zk_close.h:
// the host compiler builds the very text a kernel runs (tools/setacl_host.cpp
// puts it under ASan + UBSan on a machine without a GPU).
//   setacl_frame    the parse of a SET_ACL request body: be32 xid, be32 7,
//                   ustring path (length >= 1), an ACL vector (be32 count,
//                   then per entry be32 perms, ustring scheme, ustring id:
//                   what skip_acl walks), be32 version, and nothing behind it
//   setacl_admin    does the node's current ACL grant PERM_ADMIN to the
//                   frame's peer?
//   setacl_verdict  the answer of a well-formed or malformed frame of a served
//                   segment, ZooKeeper 3.4's order:
//                   BAD_ARGUMENTS (no request in the body) > INVALID_ACL >
//                   NO_NODE > NO_AUTH > BAD_VERSION > OK
// A segment's refusal (zk_sess.h sess_refusal) comes before all of them, with
// only the xid read (sess_xid).
// Not done, as CREATE does not do them either: no scheme or id of an entry is
// validated, equal entries are not removed, and an `auth` entry is not
// rewritten into the connection's identities (it is stored as sent and
// matches nobody, zk_auth.h).
// Every read of a frame is inside its L bytes and every read of a vector
// inside its length, whatever they hold; every loop is bounded by them.
#pragma once
#include "zk_auth.h"

namespace zk {

// A vector of this many bytes or more has no word in the ACL store
// (zk_acl.h ACL_LEN_MAX, the same number: tree_acl.hip's record pass binds
// such a CREATE lost; a SET_ACL is refused instead).
constexpr int64_t SETACL_VEC_MAX = 1 << 24;

// setacl_frame's verdicts
enum : int32_t { SF_OK = 0, SF_BAD_ARGUMENTS = 1, SF_INVALID_ACL = 2 };

struct SetAclFrame {
  int32_t status, xid, pl, version;
  int64_t poff;         // the path's bytes, absolute in buf (-1 none)
  int64_t voff, vlen;   // the vector, its count word included (-1, 0 none)
};

// Frame body [base, base + L) of buf, a SET_ACL request -> its fields.
// SF_BAD_ARGUMENTS: another opcode, a path length below 1, a length or a
// count that leaves the frame, a frame that ends before the version or goes
// on behind it.  SF_INVALID_ACL: the frame is whole, but the count is <= 0
// (nothing stands between the count and the version then) or the vector has
// SETACL_VEC_MAX bytes or more.  The spans are set only for SF_OK.
ZK_HD SetAclFrame setacl_frame(const uint8_t* __restrict__ buf, int64_t base,
                               int64_t L) {
  SetAclFrame f{SF_BAD_ARGUMENTS, 0, 0, 0, -1, -1, 0};
  if (L < 8) return f;
  const uint8_t* p = buf + base;
  f.xid = ld_be32(p);
  if (ld_be32(p + 4) != OP_SET_ACL || L < 12) return f;
  const int64_t pl = ld_be32(p + 8);
  int64_t k = 12;
  if (pl < 1 || pl > L - k) return f;
  k += pl;
  if (k + 4 > L) return f;
  const int32_t count = ld_be32(p + k);
  const int64_t v0 = k;
  k += 4;
  int64_t s = 0;
  if (count > 0) {
    s = skip_acl(p + k, L - k, count);
    if (s < 0) return f;
    k += s;
  }
  if (k + 4 != L) return f;
  if (count <= 0 || 4 + s >= SETACL_VEC_MAX) {
    f.status = SF_INVALID_ACL;
    return f;
  }
  f.status = SF_OK;
  f.pl = (int32_t)pl;
  f.version = ld_be32(p + k);
  f.poff = base + 12;
  f.voff = base + v0;
  f.vlen = 4 + s;
  return f;
}

// What the node's current ACL is to the ADMIN check: the open ACL (its word
// names arena offset 0: granted without a read of the arena), a lost binding
// (no vector: denied), or a vector to walk.
enum : int32_t { SA_OPEN = 0, SA_LOST = 1, SA_VECTOR = 2 };

// Does the node's ACL grant PERM_ADMIN to the peer at addr?  ids: the nids
// identity records of the peer's connection (zk_auth.h), or null when the
// call keeps no identity table: aclperm_permits then.  vec is read only for
// SA_VECTOR.
ZK_HD bool setacl_admin(int32_t kind, const uint8_t* __restrict__ vec,
                        int64_t len, uint32_t addr,
                        const uint8_t* __restrict__ ids, int32_t nids) {
  if (kind == SA_OPEN) return true;
  if (kind != SA_VECTOR) return false;
  return ids != nullptr
             ? aclperm_permits_auth(vec, len, PERM_ADMIN, addr, ids, nids)
             : aclperm_permits(vec, len, PERM_ADMIN, addr);
}

// The answer of a frame of a served segment.  status: setacl_frame's;
// exists: the path names a node; admin: setacl_admin's answer, or true when
// nothing is checked; version: the frame's (-1: any); aversion: the node's.
ZK_HD int32_t setacl_verdict(int32_t status, bool exists, bool admin,
                             int32_t version, int32_t aversion) {
  if (status == SF_BAD_ARGUMENTS) return ERR_BAD_ARGUMENTS;
  if (status == SF_INVALID_ACL) return ERR_INVALID_ACL;
  if (!exists) return ERR_NO_NODE;
  if (!admin) return ERR_NO_AUTH;
  if (version != -1 && version != aversion) return ERR_BAD_VERSION;
  return ERR_OK;
}

}  // namespace zk
