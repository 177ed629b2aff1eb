// The rules of the front end's device-side I/O staging (front.hip) in plain
// C++, like zk_close.h and zk_sess.h: the host compiler builds the very text
// the kernels run (tools/front_host.cpp puts it under ASan + UBSan on a
// machine without a GPU).  Three rules:
//   front_walk          how many bytes of what a connection has received are
//                       served this tick: whole frames only, a bad length ends
//                       the connection, at most `quota` frames, and either any
//                       number of non-write frames or exactly one write frame
//                       (the unordered session serve has no in-batch ordering,
//                       and a connection's requests take effect in order)
//   front_walk_ordered  the same in front of the ordered session serve: writes
//                       no longer end the run, the engines' fixed sequence does
//   front_boundary_bad  what makes the table of the raw stream's segments
//                       unsound
//   front_owner_scan,   which connection gets a watcher slot's notification
//   front_piece         slices, and the four pieces of a connection's bytes
//                       for the socket: replies, then catch-up, then
//                       write-fired, then close-fired notifications
#pragma once
#include "zk_mix.h"

namespace zk {

// A write frame, judged by its opcode word: it changes the tree (or ends the
// session), so nothing of its connection may be served beside it.
ZK_HD bool front_is_write(int32_t op) {
  return op == OP_CREATE || op == OP_DELETE || op == OP_SET_DATA ||
         op == OP_CLOSE_SESSION;
}

// take: bytes to serve this tick; nfr: the frames in them; flag: 1 = the walk
// met a bad length (nothing at or after it is taken).
struct FrontCut {
  int64_t take;
  int32_t nfr, flag;
};

// The walk over one segment of `len` bytes, be32 length + body from byte 0.
// rd(p) is the big-endian word at bytes [p, p + 4) of the segment; it is
// called with 0 <= p and p + 4 <= len only.  K1's verdict decides a bad
// length: L < 0 || L > max_packet.  A frame is a write when L >= 8 and the
// word at body + 4 says so; the walk stops before a write that is not the
// segment's first frame and after one that is.
template <class Rd>
ZK_HD FrontCut front_walk(int64_t len, int64_t quota, int64_t max_packet,
                          Rd&& rd) {
  FrontCut c{0, 0, 0};
  if (quota > 0x7fffffff) quota = 0x7fffffff;
  int64_t p = 0;
  while (c.nfr < quota && len - p >= 4) {
    const int32_t L = rd(p);
    if (L < 0 || L > max_packet) {
      c.flag = 1;
      break;
    }
    if (L > len - p - 4) break;                    // the body is not whole yet
    const bool wr = L >= 8 && front_is_write(rd(p + 8));
    if (wr && c.nfr > 0) break;
    p += 4 + (int64_t)L;
    ++c.nfr;
    if (wr) break;
  }
  c.take = p;
  return c;
}

// ---- the ordered cut ----------------------------------------------------------
// With the ordered session serve behind it (serve_sessions_mixed(ordered=True))
// a connection's writes of one batch take effect in its own order, so the run
// is no longer cut at a write.  What stays out of order inside a batch is the
// engines' fixed sequence: the list and GET_ACL engines and the SET_WATCHES
// catch-up see the tree after all the batch's writes, and the close pass runs
// after everything.  The run is the longest prefix for which that sequence is
// the connection's own order:
//   phase 0  frames of the serve's class, writes included;
//   phase 1  from the first GET_CHILDREN / GET_CHILDREN2 / GET_ACL (zk_mix.h's
//            class rule: GET_ACL only on a tree with an ACL table) or
//            SET_WATCHES frame on: a CREATE / DELETE / SET_DATA ends the run
//            before it;
//   a CLOSE_SESSION ends the run after itself.
ZK_HD bool front_is_tree_write(int32_t op) {
  return op == OP_CREATE || op == OP_DELETE || op == OP_SET_DATA;
}

ZK_HD bool front_is_late(int32_t op, bool has_acl) {
  return op == OP_GET_CHILDREN || op == OP_GET_CHILDREN2 ||
         (op == OP_GET_ACL && has_acl) || op == OP_SET_WATCHES;
}

// nwr: the write frames (front_is_write) among the nfr taken.
struct FrontCutOrd {
  int64_t take;
  int32_t nfr, flag, nwr;
};

// front_walk's contract for rd; the phase is one more word of the state.
template <class Rd>
ZK_HD FrontCutOrd front_walk_ordered(int64_t len, int64_t quota,
                                     int64_t max_packet, bool has_acl,
                                     Rd&& rd) {
  FrontCutOrd c{0, 0, 0, 0};
  if (quota > 0x7fffffff) quota = 0x7fffffff;
  int64_t p = 0;
  int32_t phase = 0;
  while (c.nfr < quota && len - p >= 4) {
    const int32_t L = rd(p);
    if (L < 0 || L > max_packet) {
      c.flag = 1;
      break;
    }
    if (L > len - p - 4) break;                    // the body is not whole yet
    const int32_t op = L >= 8 ? rd(p + 8) : 0;     // (0 is no opcode)
    if (phase == 1 && front_is_tree_write(op)) break;
    if (front_is_late(op, has_acl)) phase = 1;
    p += 4 + (int64_t)L;
    ++c.nfr;
    if (front_is_write(op)) ++c.nwr;
    if (op == OP_CLOSE_SESSION) break;
  }
  c.take = p;
  return c;
}

// ---- the cuts in front of a serve that takes SET_ACL ---------------------------
// The SET_ACL pass (tree_setacl.hip) runs behind the serve's class and in
// front of the batch's GET_ACL frames, whatever the order a connection sent
// them in.  So a SET_ACL frame (judged by its opcode word, as a write is) is
// taken only as the first frame of a connection's run and ends the run behind
// itself, in the plain and in the ordered cut: a connection's GET_ACL sent
// before its SET_ACL is answered from the old ACL, one sent after from the new,
// a tick apart.  The walks are front_walk and front_walk_ordered otherwise;
// nwr does not count a SET_ACL frame.
template <class Rd>
ZK_HD FrontCut front_walk_setacl(int64_t len, int64_t quota,
                                 int64_t max_packet, Rd&& rd) {
  FrontCut c{0, 0, 0};
  if (quota > 0x7fffffff) quota = 0x7fffffff;
  int64_t p = 0;
  while (c.nfr < quota && len - p >= 4) {
    const int32_t L = rd(p);
    if (L < 0 || L > max_packet) {
      c.flag = 1;
      break;
    }
    if (L > len - p - 4) break;                    // the body is not whole yet
    const int32_t op = L >= 8 ? rd(p + 8) : 0;     // (0 is no opcode)
    const bool wr = front_is_write(op) || op == OP_SET_ACL;
    if (wr && c.nfr > 0) break;
    p += 4 + (int64_t)L;
    ++c.nfr;
    if (wr) break;
  }
  c.take = p;
  return c;
}

template <class Rd>
ZK_HD FrontCutOrd front_walk_ordered_setacl(int64_t len, int64_t quota,
                                            int64_t max_packet, bool has_acl,
                                            Rd&& rd) {
  FrontCutOrd c{0, 0, 0, 0};
  if (quota > 0x7fffffff) quota = 0x7fffffff;
  int64_t p = 0;
  int32_t phase = 0;
  while (c.nfr < quota && len - p >= 4) {
    const int32_t L = rd(p);
    if (L < 0 || L > max_packet) {
      c.flag = 1;
      break;
    }
    if (L > len - p - 4) break;                    // the body is not whole yet
    const int32_t op = L >= 8 ? rd(p + 8) : 0;     // (0 is no opcode)
    if (op == OP_SET_ACL && c.nfr > 0) break;
    if (phase == 1 && front_is_tree_write(op)) break;
    if (front_is_late(op, has_acl)) phase = 1;
    p += 4 + (int64_t)L;
    ++c.nfr;
    if (front_is_write(op)) ++c.nwr;
    if (op == OP_CLOSE_SESSION || op == OP_SET_ACL) break;
  }
  c.take = p;
  return c;
}

// What boundary s (0..S) of raw_starts[S + 1] adds to the table-fault word on
// its own: a table that does not begin at 0, a descending pair, a boundary
// outside [0, n].  raw_starts is read at s and, for s < S, s + 1 only.
ZK_HD int32_t front_boundary_bad(const int64_t* __restrict__ raw_starts,
                                 int64_t S, int64_t n, int64_t s) {
  int32_t b = 0;
  const int64_t v = raw_starts[s];
  if (s == 0 && v != 0) ++b;
  if (v < 0 || v > n) ++b;
  if (s < S && v > raw_starts[s + 1]) ++b;
  return b;
}

// ---- the gather ---------------------------------------------------------------
// The piece holding destination byte d of a packed stream: off[P + 1] are the
// pieces' scanned offsets (off[0] = 0, d < off[P]).  The largest i < P with
// off[i] <= d, among equal offsets the last (an empty piece holds nothing);
// 0 when there is none.  off is read at an index in [0, P) only.
ZK_HD int64_t front_piece_at(const int64_t* __restrict__ off, int64_t P,
                             int64_t d) {
  int64_t lo = 0, hi = P;           // off[i] <= d for i < lo, > d from hi
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= d) lo = mid + 1;
    else hi = mid;
  }
  return lo > 0 ? lo - 1 : 0;
}

// ---- TX assembly --------------------------------------------------------------
constexpr int FRONT_SLOTS = 64;        // watcher slots of a server
constexpr int FRONT_PIECES = 4;        // pieces a connection
// the streams, in the order a connection's pieces are sent
enum : int32_t { FS_REPLY = 0, FS_RESUME = 1, FS_NOTIF = 2, FS_CLOSE = 3 };

// The owner of watcher slot w among wslots[0, cnt) (segments base ..): the
// lowest-numbered segment naming it; `named` counts the segments that do.
// Called chunk after chunk in ascending order with the same accumulators
// (owner starts at -1, named at 0).
ZK_HD void front_owner_scan(const int32_t* __restrict__ wslots, int64_t cnt,
                            int64_t base, int32_t w, int64_t& owner,
                            int64_t& named) {
  for (int64_t i = 0; i < cnt; ++i)
    if (wslots[i] == w) {
      if (owner < 0) owner = base + i;
      ++named;
    }
}

// What the pieces are cut from.  Any of rep_off, slot_off[k] and err may be
// null: an absent stream (no watch table, resume or close off, a pass that
// has no replies) has empty pieces.
struct FrontTx {
  const int64_t* rep_off;        // [S + 1] connection s's replies in stream 0
  const int64_t* slot_off[3];    // [65] watcher w's slice of streams 1..3
  int64_t cap[FRONT_PIECES];     // the streams' bytes
  const int32_t* err;            // the batch's err word
  const int32_t* wslots;         // [S]
  const int64_t* owner;          // [64] front_owner_scan's verdicts
  int64_t S;
  // [S] or null: connection s's replies end at rep_end[s], not rep_off[s + 1]
  // (the ordered serve's deferral: zk_order_clip.h clip_range).  The plain
  // front_pieces_k instance never reads it: its registers and code are what
  // they were, its kernel arguments are these 8 bytes longer.
  const int64_t* rep_end = nullptr;
};

struct FrontPiece {
  int32_t stream;
  int64_t src, len;
};

// A slice [a, b) of a stream of `cap` bytes, or nothing when the table's
// words do not describe one.
ZK_HD FrontPiece front_slice(int32_t stream, int64_t a, int64_t b,
                             int64_t cap) {
  if (a < 0 || b < a || b > cap) return FrontPiece{stream, 0, 0};
  return FrontPiece{stream, a, b - a};
}

// Piece k (0..3) of connection s < S.  Replies whatever its watcher slot is;
// slot w's slices only for a w in 0..63 whose owner is s.  rep_off is read at
// s and s + 1, a slot_off at w and w + 1, owner at w only; rep_end (END
// instances, when there) at s only.
template <bool END = true>
ZK_HD FrontPiece front_piece(const FrontTx& t, int64_t s, int32_t k) {
  const FrontPiece none{k, 0, 0};
  if (s < 0 || s >= t.S || k < 0 || k >= FRONT_PIECES) return none;
  if (t.err != nullptr && *t.err != 0) return none;
  if (k == FS_REPLY) {
    if (t.rep_off == nullptr) return none;
    if (END && t.rep_end != nullptr)
      return front_slice(k, t.rep_off[s], t.rep_end[s], t.cap[0]);
    return front_slice(k, t.rep_off[s], t.rep_off[s + 1], t.cap[0]);
  }
  const int64_t* so = t.slot_off[k - 1];
  const int32_t w = t.wslots[s];
  if (so == nullptr || w < 0 || w >= FRONT_SLOTS || t.owner[w] != s)
    return none;
  return front_slice(k, so[w], so[w + 1], t.cap[k]);
}

}  // namespace zk
