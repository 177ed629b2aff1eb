// Jute wire constants and the server-mode request parse (K12) in plain C++:
// no HIP include, so the host compiler builds the very text the kernels run
// (tools/fuzz_reqparse.cpp puts it under ASan + UBSan on a machine without
// a GPU).  zk_common.h includes this header; under hipcc every function
// here is a __host__ __device__ inline, elsewhere an inline.  parse_request
// is shared by decode_requests_k (SoA output) and the GPU server's fused
// serve (tree.hip tree_serve_k), which parses each frame in registers.
// Reference: lib/zk-consts.js:84-105 (opcodes), lib/zk-buffer.js:58-253
// (request layouts).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZK_HD __host__ __device__ __forceinline__
#else
#define ZK_HD inline
#endif

namespace zk {

// opcodes (lib/zk-consts.js:84-105; csrc/proto mirror, tests check parity)
enum : int32_t {
  OP_NOTIFICATION = 0, OP_CREATE = 1, OP_DELETE = 2, OP_EXISTS = 3,
  OP_GET_DATA = 4, OP_SET_DATA = 5, OP_GET_ACL = 6, OP_SET_ACL = 7,
  OP_GET_CHILDREN = 8, OP_SYNC = 9, OP_PING = 11, OP_GET_CHILDREN2 = 12,
  OP_CHECK = 13, OP_MULTI = 14, OP_AUTH = 100, OP_SET_WATCHES = 101,
  OP_SASL = 102, OP_CREATE_SESSION = -10, OP_CLOSE_SESSION = -11,
  OP_ERROR = -1, OP_UNKNOWN = -1000
};
enum : int32_t {
  XID_NOTIFICATION = -1, XID_PING = -2, XID_AUTH = -4, XID_SET_WATCHES = -8
};
enum : int32_t { ERR_OK = 0, ERR_SYSTEM = -1, ERR_UNIMPLEMENTED = -6,
                 ERR_BAD_ARGUMENTS = -8, ERR_NO_NODE = -101,
                 ERR_BAD_VERSION = -103, ERR_NO_CHILDREN_FOR_EPHEMERALS = -108,
                 ERR_NODE_EXISTS = -110, ERR_NOT_EMPTY = -111,
                 ERR_SESSION_EXPIRED = -112, ERR_INVALID_ACL = -114 };
// per-record decode status
enum : int32_t { ST_OK = 0, ST_BAD_DECODE = 1, ST_NO_XID = 2,
                 ST_BAD_OPCODE = 3 };

ZK_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
ZK_HD uint64_t bswap64(uint64_t v) { return __builtin_bswap64(v); }

ZK_HD int32_t ld_be32(const uint8_t* p) {
  uint32_t v; __builtin_memcpy(&v, p, 4); return (int32_t)bswap32(v);
}
ZK_HD int64_t ld_be64(const uint8_t* p) {
  uint64_t v; __builtin_memcpy(&v, p, 8); return (int64_t)bswap64(v);
}

// Walk `count` ustrings starting at p; returns bytes consumed or -1.
ZK_HD int64_t skip_strings(const uint8_t* p, int64_t avail, int32_t count) {
  int64_t k = 0;
  for (int32_t j = 0; j < count; ++j) {
    if (k + 4 > avail) return -1;
    int32_t l = ld_be32(p + k);
    if (l < 0) l = 0;
    // (64-bit: a length word of 2^31 - 4 .. 2^31 - 1 overflowed `4 + l` as
    // int and sent k, and the next load, 2 GiB below the frame)
    k += 4 + (int64_t)l;
    if (k > avail) return -1;
  }
  return k;
}

// ACL vector entries: perms i32, scheme ustring, id ustring.
ZK_HD int64_t skip_acl(const uint8_t* p, int64_t avail, int32_t count) {
  int64_t k = 0;
  for (int32_t j = 0; j < count; ++j) {
    if (k + 4 > avail) return -1;
    k += 4;
    int64_t s = skip_strings(p + k, avail - k, 2);
    if (s < 0) return -1;
    k += s;
  }
  return k;
}

struct ReqFields {
  int32_t status, xid, op, arg, pl, dl, vc;
  int64_t poff, doff, voff, rel;
};

// Frame body [base, base + L) of buf -> the request's fields (offsets are
// absolute in buf).
ZK_HD ReqFields parse_request(const uint8_t* __restrict__ buf, int64_t base,
                              int64_t L) {
  const uint8_t* p = buf + base;
  int32_t status = ST_OK, xid = 0, op = OP_UNKNOWN, arg = 0;
  int64_t poff = -1, doff = -1, voff = -1, rel = 0;
  int32_t pl = 0, dl = 0, vc = 0;
  if (L < 8) {
    status = ST_BAD_DECODE;
  } else {
    xid = ld_be32(p);
    op = ld_be32(p + 4);
    int64_t k = 8;
    auto get_str = [&](int64_t& off, int32_t& len) -> bool {
      if (k + 4 > L) return false;
      int32_t l = ld_be32(p + k);
      if (l < 0) l = 0;
      if (k + 4 + l > L) return false;
      off = base + k + 4;
      len = l;
      k += 4 + l;
      return true;
    };
    auto get_i32 = [&](int32_t& v) -> bool {
      if (k + 4 > L) return false;
      v = ld_be32(p + k);
      k += 4;
      return true;
    };
    bool ok = true;
    switch (op) {
      case OP_GET_DATA: case OP_EXISTS: case OP_GET_CHILDREN:
      case OP_GET_CHILDREN2:
        ok = get_str(poff, pl) && k + 1 <= L;
        if (ok) { arg = p[k]; ok = (arg == 0 || arg == 1); ++k; }
        break;
      case OP_CREATE: {
        ok = get_str(poff, pl) && get_str(doff, dl) && get_i32(vc);
        if (!ok) break;
        if (vc < 0) vc = 0;
        voff = base + k;
        const int64_t s = skip_acl(p + k, L - k, vc);
        ok = s >= 0;
        if (ok) { k += s; ok = get_i32(arg); }
        break;
      }
      case OP_DELETE:
        ok = get_str(poff, pl) && get_i32(arg);
        break;
      case OP_SET_DATA:
        ok = get_str(poff, pl) && get_str(doff, dl) && get_i32(arg);
        break;
      case OP_GET_ACL: case OP_SYNC:
        ok = get_str(poff, pl);
        break;
      case OP_SET_WATCHES: {
        if (k + 8 > L) { ok = false; break; }
        rel = ld_be64(p + k);
        k += 8;
        voff = base + k;
        for (int g = 0; g < 3 && ok; ++g) {
          int32_t c;
          ok = get_i32(c);
          if (!ok) break;
          if (c < 0) c = 0;
          const int64_t s = skip_strings(p + k, L - k, c);
          ok = s >= 0;
          if (!ok) break;      // (c is unbounded here: vc + c may overflow)
          k += s;
          vc += c;
        }
        break;
      }
      case OP_PING: case OP_CLOSE_SESSION:
        break;
      default:
        status = ST_BAD_OPCODE;
    }
    if (!ok) status = ST_BAD_DECODE;
  }
  return ReqFields{status, xid, op, arg, pl, dl, vc, poff, doff, voff, rel};
}

}  // namespace zk
