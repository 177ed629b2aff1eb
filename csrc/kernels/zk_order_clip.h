// The rules of the ordered session serve's deferral (tree_order.hip
// ord_clip_*) in plain C++, like zk_front.h and zk_close.h: the host compiler
// builds the very text the kernels run (tools/order_clip_host.cpp puts it
// under ASan + UBSan on a machine without a GPU).
//
// An ordered serve of `passes` launches cannot apply a request whose rank (the
// longest chain of conflicting earlier requests of the batch) is >= passes.
// A library answers it SYSTEMERROR; a network server must not.  So the frame
// and everything after it in its connection (segment) is deferred: it is
// taken out of the batch before the first serve pass, answered nothing, and
// its bytes stay with the connection for the next batch.  Three rules:
//   clip_overflow   is this frame of the whole batch one the passes cannot
//                   reach
//   clip_deferred   is it deferred, given clipf[S]: per segment the smallest
//                   whole-batch index of an overflowing frame (ncap: none)
//   clip_range      per segment, where its replies end in the merged reply
//                   stream and how many of its request bytes were consumed
#pragma once
#include "zk_mix.h"

namespace zk {

constexpr int32_t CLIP_RANK = 0x7f;    // the rank bits of a rank byte

// Frame i of the whole batch, of class cls and index sub in its class's
// compacted table; rank[ncap] is the ordering pass's byte per frame of the
// serve's class.  rank is read at sub only, and only for 0 <= sub < ncap.
ZK_HD bool clip_overflow(int32_t cls, int32_t sub,
                         const uint8_t* __restrict__ rank, int64_t ncap,
                         int32_t passes) {
  if (cls != MIX_A || sub < 0 || sub >= ncap) return false;
  return (int32_t)(rank[sub] & CLIP_RANK) >= passes;
}

// A frame of no segment (seg outside [0, S)) is refused as it is, not
// deferred.  clipf is read at seg only.
ZK_HD bool clip_deferred(const int64_t* __restrict__ clipf, int64_t S,
                         int64_t seg, int64_t i) {
  return seg >= 0 && seg < S && i >= clipf[seg];
}

struct ClipRange {
  int64_t rep_end;   // the segment's replies: out[rep_off[s], rep_end)
  int64_t used;      // request bytes of the segment that were consumed
};

// Segment s < S of a batch of nfr frames (the device count clipped to ncap).
// rep_off[S + 1]: sess_ranges' slices of the merged stream; rec_off[ncap]:
// the merged reply starts; off[ncap]: the frames' bodies in rx (a frame starts
// 4 bytes before its body); starts[S + 1]: the segments' bytes.  A segment is
// clipped when clipf[s] is in [0, nfr).  rec_off and off are read at clipf[s]
// only, and only then; both results stay inside the segment's own slice
// whatever the tables hold.
ZK_HD ClipRange clip_range(const int64_t* __restrict__ clipf,
                           const int64_t* __restrict__ rep_off,
                           const int64_t* __restrict__ rec_off,
                           const int64_t* __restrict__ off,
                           const int64_t* __restrict__ starts, int64_t nfr,
                           int64_t s) {
  const int64_t r0 = rep_off[s], r1 = rep_off[s + 1];
  const int64_t b0 = starts[s], b1 = starts[s + 1];
  ClipRange r{r1, b1 > b0 ? b1 - b0 : 0};
  const int64_t c = clipf[s];
  if (c < 0 || c >= nfr) return r;
  int64_t e = rec_off[c];
  if (e > r1) e = r1;
  if (e < r0) e = r0;
  int64_t u = off[c] - 4 - b0;
  if (u > r.used) u = r.used;
  if (u < 0) u = 0;
  r.rep_end = e;
  r.used = u;
  return r;
}

}  // namespace zk
