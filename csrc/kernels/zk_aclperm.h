// The rule of ACL enforcement in a session batch (tree_aclperm.hip) in plain
// C++, like zk_close.h and zk_sess.h: the host compiler builds the very text
// the kernels run (tools/aclperm_host.cpp puts it under ASan + UBSan on a
// machine without a GPU).  Three rules:
//   aclperm_need      the permission bit an op needs and the node it is
//                     checked on (ZooKeeper 3.4 / 3.5: the servers the
//                     reference client talks to)
//   aclperm_ip_match  ZooKeeper's `ip` provider: does an `a.b.c.d[/bits]` id
//                     cover the peer's IPv4 address?
//   aclperm_permits   a bounded walk over one ACL vector in wire format
//                     (be32 count, then per entry be32 perms, ustring scheme,
//                     ustring id): does any entry both match the peer and
//                     carry the bit?
// Every read of a vector or an id is inside its `len` bytes, whatever they
// hold; every loop is bounded by those bytes.
#pragma once
#include "zk_wire.h"

namespace zk {

constexpr int32_t ERR_NO_AUTH = -102;

// ZooDefs.Perms
enum : int32_t { PERM_READ = 1, PERM_WRITE = 2, PERM_CREATE = 4,
                 PERM_DELETE = 8, PERM_ADMIN = 16 };

// Where the bit is looked for: nowhere (the op needs no permission), on the
// node the path names, on its parent, or on its parent and only when the node
// itself exists (DELETE: a missing node answers NO_NODE whatever the parent
// allows).
enum : int32_t { ACLT_NONE = 0, ACLT_NODE = 1, ACLT_PARENT = 2,
                 ACLT_PARENT_OF_NODE = 3 };

struct AclNeed {
  int32_t perm, target;
};

ZK_HD AclNeed aclperm_need(int32_t op) {
  switch (op) {
    case OP_GET_DATA: case OP_GET_CHILDREN: case OP_GET_CHILDREN2:
      return AclNeed{PERM_READ, ACLT_NODE};
    case OP_SET_DATA:
      return AclNeed{PERM_WRITE, ACLT_NODE};
    case OP_CREATE:
      return AclNeed{PERM_CREATE, ACLT_PARENT};
    case OP_DELETE:
      return AclNeed{PERM_DELETE, ACLT_PARENT_OF_NODE};
    default:        // EXISTS, GET_ACL, SYNC, PING, SET_WATCHES, CLOSE_SESSION...
      return AclNeed{0, ACLT_NONE};
  }
}

// Up to `most + 1` decimal digits of id[k, len) -> v, k moved past them;
// returns how many were read (most + 1: too many).
ZK_HD int32_t aclperm_digits(const uint8_t* __restrict__ id, int64_t len,
                             int64_t& k, int32_t most, int32_t& v) {
  int32_t nd = 0;
  v = 0;
  while (k < len && nd <= most && id[k] >= '0' && id[k] <= '9') {
    v = v * 10 + (id[k] - '0');
    ++nd;
    ++k;
  }
  return nd;
}

// Does the `ip` id [id, id + len) cover addr (a host-order IPv4 address)?
// The id is a.b.c.d or a.b.c.d/bits: exactly four parts of 1-3 digits, each
// <= 255; bits 1-2 digits, <= 32 (32 without the suffix); the first `bits`
// bits of the two addresses are compared.  Anything else matches nothing, and
// addr 0 ("no IPv4 identity") matches no id.
ZK_HD bool aclperm_ip_match(const uint8_t* __restrict__ id, int64_t len,
                            uint32_t addr) {
  if (addr == 0 || len <= 0) return false;
  int64_t k = 0;
  uint32_t ip = 0;
  for (int part = 0; part < 4; ++part) {
    int32_t v;
    const int32_t nd = aclperm_digits(id, len, k, 3, v);
    if (nd < 1 || nd > 3 || v > 255) return false;
    ip = (ip << 8) | (uint32_t)v;
    if (part < 3) {
      if (k >= len || id[k] != '.') return false;
      ++k;
    }
  }
  int32_t bits = 32;
  if (k < len) {
    if (id[k] != '/') return false;
    ++k;
    const int32_t nd = aclperm_digits(id, len, k, 2, bits);
    if (nd < 1 || nd > 2 || bits > 32 || k != len) return false;
  }
  const uint32_t mask = bits == 0 ? 0u : 0xFFFFFFFFu << (32 - bits);
  return ((ip ^ addr) & mask) == 0;
}

ZK_HD bool aclperm_is(const uint8_t* __restrict__ p, int64_t n,
                      const char* lit, int64_t m) {
  if (n != m) return false;
  for (int64_t k = 0; k < m; ++k)
    if (p[k] != (uint8_t)lit[k]) return false;
  return true;
}

// Does the vector [vec, vec + len) grant `perm` to a peer at addr?  world
// matches with the id "anyone" only, ip as above; every other scheme (digest,
// auth, sasl, ...) matches nobody: the peer here has no identity but its
// address (zk_auth.h aclperm_permits_auth: one that holds digest identities).
// A count or a
// length that leaves the vector ends the walk: denied.  (A negative string
// length is Jute's null string: empty, as skip_acl takes it.)
ZK_HD bool aclperm_permits(const uint8_t* __restrict__ vec, int64_t len,
                           int32_t perm, uint32_t addr) {
  if (len < 4) return false;
  const int32_t n = ld_be32(vec);
  int64_t k = 4;
  for (int32_t j = 0; j < n; ++j) {
    // (every entry takes 12 bytes or more: the walk ends inside len)
    if (k + 8 > len) return false;
    const int32_t perms = ld_be32(vec + k);
    int64_t sl = ld_be32(vec + k + 4);
    k += 8;
    if (sl < 0) sl = 0;
    if (sl > len - k) return false;
    const uint8_t* scheme = vec + k;
    k += sl;
    if (k + 4 > len) return false;
    int64_t il = ld_be32(vec + k);
    k += 4;
    if (il < 0) il = 0;
    if (il > len - k) return false;
    const uint8_t* id = vec + k;
    k += il;
    if ((perms & perm) == 0) continue;
    if (aclperm_is(scheme, sl, "world", 5)) {
      if (aclperm_is(id, il, "anyone", 6)) return true;
    } else if (aclperm_is(scheme, sl, "ip", 2)) {
      if (aclperm_ip_match(id, il, addr)) return true;
    }
  }
  return false;
}

// The parent path of path [p, p + pl): its first `cut` bytes, as do_create
// cuts it; 0: a child of the root (which has no node in this tree) or no path.
ZK_HD int32_t aclperm_parent_cut(const uint8_t* __restrict__ p, int32_t pl) {
  int32_t cut = pl - 1;
  while (cut > 0 && p[cut] != '/') --cut;
  return cut > 0 ? cut : 0;
}

}  // namespace zk
