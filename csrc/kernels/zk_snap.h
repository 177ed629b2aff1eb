// The tree image (version 1): the byte layout GpuTree.snapshot writes and
// GpuTree.load reads (tree_snap.hip), and its structural checks, in plain
// C++ like zk_wire.h: the host compiler builds the very text the load's
// check kernel runs (tools/fuzz_snap.cpp puts it under ASan + UBSan on a
// machine without a GPU).  zkmi/utils/treeimage.py is the host mirror.
//
//   header   64 bytes, little-endian (SH_* below)
//   table    int64 rec_off[n + 1], little-endian, relative to the body:
//            rec_off[0] = 0, rec_off[n] = body_bytes, strictly increasing,
//            multiples of 8
//   body     record i at rec_off[i], Jute wire format (big-endian), zero
//            padded to 8 bytes:
//              be32 path_len, path
//              Stat (68 bytes)
//              be32 data_len (>= 0), data
//              be32 ACL count, entries (perms, scheme, id); count -1: the
//              node's ACL binding was lost
//
// Records are in ascending node index of the tree they came from; a loaded
// tree places record i at node i.  Nothing in an image is a pointer or a
// tree offset.
#pragma once
#include "zk_wire.h"

namespace zk {

constexpr int64_t SNAP_HEAD = 64;
constexpr uint32_t SNAP_VERSION = 1;
// header fields (byte offsets)
enum : int { SH_MAGIC = 0, SH_VERSION = 8, SH_RESERVED = 12, SH_N = 16,
             SH_BODY = 24, SH_ZXID = 32, SH_DIGEST = 40, SH_PATH16 = 48,
             SH_MAX_DATA = 56 };
// "ZKMITREE" as the little-endian word at SH_MAGIC
constexpr uint64_t SNAP_MAGIC = 0x45455254494D4B5Aull;

// Outcome of a load, in check order (the earliest failing phase and the
// smallest record index failing in it are reported; NO_ROOM and DIGEST
// carry index -1).  snapshot(out=...) reports SNAP_NO_ROOM too.
// SNAP_DUP_PATH means two records of one path, byte for byte: distinct paths
// of one 64-bit hash key load, however many of them share a wave (the index
// build's second launch, tree_snap.hip).
enum : int32_t { SNAP_OK = 0, SNAP_BAD_HEADER = 1, SNAP_BAD_TABLE = 2,
                 SNAP_BAD_RECORD = 3, SNAP_NO_ROOM = 4, SNAP_DUP_PATH = 5,
                 SNAP_ORPHAN = 6, SNAP_DIGEST = 7 };

constexpr int32_t SNAP_STAT = 68;
// paths fit the tree's path word (offset << 24 | length), ACL vectors the
// ACL table's
constexpr int64_t SNAP_PATH_MAX = (1 << 24) - 1;
constexpr int64_t SNAP_ACL_MAX = (1 << 24) - 1;
// ZooKeeper's open ACL (world:anyone, all permissions) in wire format
constexpr int32_t SNAP_OPEN_ACL_BYTES = 27;

ZK_HD int64_t ld_le64(const uint8_t* p) {
  int64_t v; __builtin_memcpy(&v, p, 8); return v;
}
ZK_HD uint32_t ld_le32(const uint8_t* p) {
  uint32_t v; __builtin_memcpy(&v, p, 4); return v;
}
ZK_HD int64_t snap_pad8(int64_t x) { return (x + 7) & ~(int64_t)7; }
ZK_HD int64_t snap_pad16(int64_t x) { return (x + 15) & ~(int64_t)15; }

struct SnapHead {
  int64_t n, body, zxid, path16, max_data;
  uint64_t digest;
};

// The header and the table's frame of image img[0, len): SNAP_OK,
// SNAP_BAD_HEADER or (an image of no record whose rec_off[0] is not 0)
// SNAP_BAD_TABLE.  Reads nothing at or past len.  On SNAP_OK the table
// (n + 1 words at SNAP_HEAD) and the body (h->body bytes behind it) lie
// inside the image.
ZK_HD int32_t snap_check_header(const uint8_t* img, int64_t len, SnapHead* h) {
  if (len < SNAP_HEAD) return SNAP_BAD_HEADER;
  if ((uint64_t)ld_le64(img + SH_MAGIC) != SNAP_MAGIC) return SNAP_BAD_HEADER;
  if (ld_le32(img + SH_VERSION) != SNAP_VERSION) return SNAP_BAD_HEADER;
  h->n = ld_le64(img + SH_N);
  h->body = ld_le64(img + SH_BODY);
  h->zxid = ld_le64(img + SH_ZXID);
  h->digest = (uint64_t)ld_le64(img + SH_DIGEST);
  h->path16 = ld_le64(img + SH_PATH16);
  h->max_data = ld_le64(img + SH_MAX_DATA);
  const int64_t room = len - SNAP_HEAD;           // table + body
  if (h->n < 0 || h->n > room / 8 - 1) return SNAP_BAD_HEADER;
  const int64_t left = room - 8 * (h->n + 1);
  if (h->body < 0 || (h->body & 7) != 0 || h->body > left)
    return SNAP_BAD_HEADER;
  if (h->n == 0) {
    if (h->body != 0) return SNAP_BAD_HEADER;
    if (ld_le64(img + SNAP_HEAD) != 0) return SNAP_BAD_TABLE;
  }
  return SNAP_OK;
}

// Entry i < n of the table tab[0, n + 1] of a body of `body` bytes: its
// span [tab[i], tab[i + 1]) is non-empty, 8-aligned and inside the body,
// the first one starts at 0 and the last one ends the body.
ZK_HD bool snap_check_table(const uint8_t* tab, int64_t n, int64_t body,
                            int64_t i) {
  const int64_t a = ld_le64(tab + 8 * i), b = ld_le64(tab + 8 * (i + 1));
  if (i == 0 && a != 0) return false;
  if (i == n - 1 && b != body) return false;
  if (((a | b) & 7) != 0) return false;
  return a >= 0 && a < b && b <= body;
}

// What the record check found: the field offsets inside the record.
struct SnapRec {
  int32_t pl, dl;
  int32_t acl_count;          // -1: a lost binding
  int64_t path, stat, data, acl, acl_len;   // acl: at its count word
};

// Record r[0, span): true when it is a whole record of exactly `span` bytes
// (the zero padding to 8 included).  Every read is bounded by span.
ZK_HD bool snap_check_record(const uint8_t* r, int64_t span, SnapRec* o) {
  int64_t k = 0;
  if (k + 4 > span) return false;
  const int32_t pl = ld_be32(r + k);
  k += 4;
  if (pl < 2 || (int64_t)pl > SNAP_PATH_MAX || k + pl > span) return false;
  if (r[k] != '/' || r[k + pl - 1] == '/') return false;
  o->pl = pl;
  o->path = k;
  k += pl;
  if (k + SNAP_STAT > span) return false;
  o->stat = k;
  k += SNAP_STAT;
  if (k + 4 > span) return false;
  const int32_t dl = ld_be32(r + k);
  k += 4;
  if (dl < 0 || k + dl > span) return false;
  if (ld_be32(r + o->stat + 52) != dl) return false;     // Stat.dataLength
  o->dl = dl;
  o->data = k;
  k += dl;
  if (k + 4 > span) return false;
  const int32_t cnt = ld_be32(r + k);
  o->acl = k;
  o->acl_count = cnt;
  k += 4;
  if (cnt < -1 || cnt == 0) return false;
  if (cnt > 0) {
    const int64_t s = skip_acl(r + k, span - k, cnt);
    if (s < 0 || 4 + s > SNAP_ACL_MAX) return false;
    k += s;
  }
  o->acl_len = k - o->acl;
  if (snap_pad8(k) != span) return false;
  for (; k < span; ++k)
    if (r[k] != 0) return false;
  return true;
}

}  // namespace zk
