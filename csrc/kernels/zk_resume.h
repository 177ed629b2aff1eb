// The SET_WATCHES catch-up of a session batch (tree_resume.hip) in plain C++,
// like zk_sess.h and zk_mix.h: the host compiler builds the very text the
// kernels run (tools/resume_host.cpp puts it under ASan + UBSan on a machine
// without a GPU).  Three rules:
//   resume_frame    which frames of a batch are caught up, and for whom
//   resume_walk     the listing walk over a SET_WATCHES body: three lists of
//                   `be32 count, count x (be32 length, bytes)`
//   resume_decide   what a listed path gets (SURVEY Appendix D,
//                   lib/zk-session.js:421-471): the table of wt_resume_k
//
// The walk is wt_resume_k's (tree_watch.hip): a count or a length that runs
// past the frame ends the frame's listing, the paths listed before it stand,
// negative counts and lengths read as 0.  It is written as a machine that is
// fed the frame a piece at a time, so the kernel can stage the frame through
// LDS in chunks while the host runs it over the whole frame at once: every
// word is read through `rd(k)`, only for k with first <= k and k + 4 <=
// avail <= end, whatever the words say.
#pragma once
#include "zk_sess.h"

namespace zk {

// The kernel's staging chunk (bytes; a wave's 16-byte loads of one
// instruction).  Chunk c of a frame covers rx[c0 + c * RS_CHUNK, ...), c0 =
// the list start (frame body + 16) rounded down to 16.
constexpr int64_t RS_CHUNK = 1024;
// body: xid, opcode, relZxid, and at least the first count
constexpr int64_t RS_HEAD = 16;

enum : int32_t { RL_DATA = 0, RL_EXIST = 1, RL_CHILD = 2 };
// notification types (lib/zk-consts.js) as the events carry them
enum : int32_t { RN_CREATED = 1, RN_DELETED = 2, RN_DATA_CHANGED = 3,
                 RN_CHILDREN_CHANGED = 4 };
// what a listed path gets: an event type above, or
constexpr int32_t RD_ARM_DATA = -1, RD_ARM_CHILD = -2;

// What frame j (body [off, off + L) of rx[0, rx_len), segment seg) is for the
// catch-up: its watcher slot (0..63), RF_NONE (not caught up, not counted) or
// RF_NO_SLOT (a live SET_WATCHES frame whose segment has no valid watcher
// slot: its paths are counted, nothing else).  seg_state and wslots are read
// at an index in [0, S) only, rx inside [off, off + 8) only and only when
// the body lies inside rx.
constexpr int32_t RF_NONE = -1, RF_NO_SLOT = -2;
ZK_HD int32_t resume_frame(const uint8_t* __restrict__ rx, int64_t rx_len,
                           int64_t off, int64_t L,
                           const int64_t* __restrict__ bad,
                           const int32_t* __restrict__ seg_state,
                           const int32_t* __restrict__ wslots, int64_t S,
                           int64_t seg) {
  if (sess_refusal(bad, seg_state, S, seg) != ERR_OK) return RF_NONE;
  if (off < 0 || L < RS_HEAD + 4 || off > rx_len || L > rx_len - off)
    return RF_NONE;
  if (ld_be32(rx + off + 4) != OP_SET_WATCHES) return RF_NONE;
  const int32_t w = wslots[seg];
  return w >= 0 && w < 64 ? w : RF_NO_SLOT;
}

// The walk's state.  k: the next word (an offset in rx); g: the list (3:
// past the last); left: paths of list g still to come; m: paths listed.
// done: nothing more will be listed; ok (once done): the three lists were
// whole — what parse_request calls a well-formed SET_WATCHES.
struct ResumeWalk {
  int64_t k, m;
  int32_t g, left;
  bool want_count, done, ok;
};

ZK_HD ResumeWalk resume_walk_begin(int64_t body_off) {
  return ResumeWalk{body_off + RS_HEAD, 0, 0, 0, true, false, false};
}

// Advance over the bytes before `avail` (<= end = the frame's end).  rd(k):
// the big-endian word at rx[k, k + 4); emit(m, kind, off, len): path m.
template <class Rd, class Emit>
ZK_HD void resume_walk(ResumeWalk& w, int64_t avail, int64_t end, Rd rd,
                       Emit emit) {
  while (!w.done) {
    if (w.g >= 3) {
      w.done = w.ok = true;
      break;
    }
    if (w.k + 4 > end) {              // a count or a length cut by the frame
      w.done = true;
      break;
    }
    if (w.k + 4 > avail) break;       // the word is not staged yet
    int32_t v = rd(w.k);
    if (v < 0) v = 0;
    if (w.want_count) {
      w.k += 4;
      w.left = v;
      w.want_count = false;
    } else {
      if (w.k + 4 + (int64_t)v > end) {   // a path cut by the frame
        w.done = true;
        break;
      }
      emit(w.m, w.g, w.k + 4, v);
      ++w.m;
      w.k += 4 + (int64_t)v;
      --w.left;
    }
    if (w.left == 0) {
      ++w.g;
      w.want_count = true;
    }
  }
}

// The session rule.  there: the node exists; mzxid, pzxid: its (unread when
// it does not); rel: the frame's relZxid.
ZK_HD int32_t resume_decide(int32_t kind, bool there, int64_t mzxid,
                            int64_t pzxid, int64_t rel) {
  if (kind == RL_DATA) {
    if (!there) return RN_DELETED;
    return mzxid > rel ? RN_DATA_CHANGED : RD_ARM_DATA;
  }
  if (kind == RL_EXIST) return there ? RN_CREATED : RD_ARM_DATA;
  if (!there) return RN_DELETED;
  return pzxid > rel ? RN_CHILDREN_CHANGED : RD_ARM_CHILD;
}

// The frame of entry e: the largest j < nf with base[j] <= e (among equal
// bases the last one: a frame that lists nothing owns nothing); -1 if none.
// base is read at an index in [0, nf) only.
ZK_HD int64_t resume_entry_frame(const int64_t* __restrict__ base, int64_t nf,
                                 int64_t e) {
  int64_t lo = 0, hi = nf;          // base[j] <= e for j < lo, > e from hi
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (base[mid] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

}  // namespace zk
