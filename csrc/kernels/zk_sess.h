// The segment rule of a session batch (tree_sess.hip), in plain C++ like
// zk_wire.h and zk_mix.h: the host compiler builds the very text the kernels
// run (tools/sess_host.cpp puts it under ASan + UBSan on a machine without a
// GPU).
//
// A batch rx[:n] carries the whole frames of S connections, concatenated.
// Its segment table: starts[S + 1] (byte offsets into rx, non-decreasing,
// starts[0] = 0), and per segment a session and a watcher slot.  Frame j of
// K1's table (body offset off_j, body length len_j) has its header at
// h_j = off_j - 4 and ends at e_j = off_j + len_j.
//   seg(j)    the largest s < S with starts[s] <= h_j (among equal starts the
//             last one: an empty segment owns nothing); -1 if there is none
//   torn      seg(j) < 0 or e_j > starts[seg(j) + 1]
//   first[s]  the number of frames with h_j < starts[s], s in 0..S
// Every read of starts is at an index in [0, S], every read of off at an
// index in [0, nf): whatever the tables hold.  Values are int64 throughout.
#pragma once
#include "zk_wire.h"

namespace zk {

// seg(j) for a header at h.
ZK_HD int64_t sess_seg(const int64_t* __restrict__ starts, int64_t S,
                       int64_t h) {
  int64_t lo = 0, hi = S;           // starts[s] <= h for s < lo, > h from hi
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (starts[mid] <= h) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// Is the frame ending at e, of segment seg = sess_seg(...), torn?
ZK_HD bool sess_torn(const int64_t* __restrict__ starts, int64_t S,
                     int64_t seg, int64_t e) {
  if (seg < 0 || seg >= S) return true;
  return e > starts[seg + 1];
}

// first[s] for the boundary at byte `start`: the frames (off[0, nf), in
// stream order) whose header lies before it.
ZK_HD int64_t sess_first(const int64_t* __restrict__ off, int64_t nf,
                         int64_t start) {
  int64_t lo = 0, hi = nf;          // off[j] - 4 < start for j < lo
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] - 4 < start) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// What boundary s (0..S) adds to `bad` on its own: a descending pair
// starts[s] > starts[s + 1] (s < S), and a table that does not start at 0.
ZK_HD int32_t sess_boundary_bad(const int64_t* __restrict__ starts, int64_t S,
                                int64_t s) {
  int32_t b = 0;
  if (s == 0 && starts[0] != 0) ++b;
  if (s < S && starts[s] > starts[s + 1]) ++b;
  return b;
}

// ---- a session batch of any op mix (GpuServer.serve_sessions_mixed) ---------
// The list and GET_ACL engines' session instances (tree_list.hip,
// tree_acl.hip) take a frame's segment from the table the split-segments
// pass (tree_sess.hip sess_split_seg_k) compacted beside the class's frame
// table.  What they and that pass decide from hostile tables is here.

// Is v an index into a table of n entries?
ZK_HD bool sess_in(int64_t v, int64_t n) { return v >= 0 && v < n; }

// What a frame of segment `seg` is refused with before anything of it but
// the xid is read: SYSTEMERROR when the table is unsound (*bad != 0) or the
// segment is none of its S, SESSION_EXPIRED when its session is not alive
// (seg_state[seg] == 1), else OK.  seg_state is read at an index in [0, S)
// only.
ZK_HD int32_t sess_refusal(const int64_t* __restrict__ bad,
                           const int32_t* __restrict__ seg_state, int64_t S,
                           int64_t seg) {
  if (*bad != 0 || !sess_in(seg, S)) return ERR_SYSTEM;
  return seg_state[seg] == 1 ? ERR_SESSION_EXPIRED : ERR_OK;
}

// The xid of a refused frame: what parse_request gives (0 for a body without
// one).
ZK_HD int32_t sess_xid(const uint8_t* __restrict__ buf, int64_t base,
                       int64_t L) {
  return L < 8 ? 0 : ld_be32(buf + base);
}

// The split-segments rule: frame i of class cls, index sub inside it, puts
// its segment at f_seg_c[cls][sub], three tables of ncap entries.  A class
// outside 0..2 or an index outside [0, ncap) has no place: -1; else the
// place in the tables laid end to end, cls * ncap + sub.
ZK_HD int64_t sess_split_at(int64_t cls, int64_t sub, int64_t ncap) {
  if (!sess_in(cls, 3) || !sess_in(sub, ncap)) return -1;
  return cls * ncap + sub;
}

// The segment table as the list and GET_ACL session instances read it.
struct SegTable {
  const int32_t* f_seg;      // [ncap] the class's frame -> segment
  const int32_t* wslots;     // [S]
  const int32_t* seg_state;  // [S] 0 serve, 1 session not alive
  const int64_t* bad;        // [2] != 0: the table is unsound
  int64_t S;
};

}  // namespace zk
