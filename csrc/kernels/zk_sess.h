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

}  // namespace zk
