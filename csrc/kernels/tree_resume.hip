// SET_WATCHES catch-up for a whole session batch (GpuServer.serve_sessions /
// serve_sessions_mixed with resume=True; the rules: zk_resume.h).  Every
// SET_WATCHES frame of the batch is caught up for its own segment's watcher
// slot, against the tree as the batch left it: what changed after the
// frame's relZxid becomes an xid -1 event, the other watches are re-armed.
// The passes:
//   rs_list_k<false>   a wave per frame: is it caught up (resume_frame), and
//                      how many paths does it list.  The frame is staged
//                      through LDS in RS_CHUNK pieces, coalesced 16-byte
//                      loads, the next piece's loads issued before the walk
//                      of this one starts; the serial walk over `be32 length
//                      + bytes` (resume_walk) reads LDS, not a dependent trip
//                      to HBM per path.  A frame that is not caught up, and
//                      one whose lists are not whole, counts 0 — so frame
//                      order is stream order with no compaction pass, and the
//                      well-formedness is the walk's own verdict (what
//                      parse_request decides, without a second serial walk
//                      from global memory).
//   (the device-wide scan of the counts: each frame's base)
//   rs_list_k<true>    the same walk, writing (kind, offset, length) entries
//                      at the frame's base
//   rs_decide_k        a lane per entry: its frame by binary search over the
//                      bases, the frame's segment, watcher slot and relZxid,
//                      the lookup, the rule (resume_decide); re-arm with
//                      wt_arm, or flag one event
//   (the device-wide scan of the flags)
//   rs_emit_k          (slot, type, path) records in entry order
// and zk_sess_group_events (tree_sess.hip) groups them by watcher slot.  No
// lane waits for another's store; the only atomics are wt_arm's and the stats
// counters', one a wave.
#include "zk_tree.h"
#include "zk_resume.h"

namespace zk {

constexpr int RS_T = WAVE;            // the list passes: a wave a workgroup
constexpr int RD_T = 256;
constexpr int RS_RING = 2 * RS_CHUNK / 4;     // words of the LDS ring
static_assert(RS_CHUNK == RS_T * 16, "a chunk is one 16-byte load a lane");
static_assert((RS_RING & (RS_RING - 1)) == 0, "the ring index is masked");

// stats[]: what GpuServer.resume_stats reports
enum : int { RST_EVENTS = 0, RST_WRITTEN = 1, RST_REARMED = 2, RST_LISTED = 3,
             RST_DROPPED = 4, RST_NO_SLOT = 5, RST_N = 8 };

struct RsBatch {
  const uint8_t* rx;
  int64_t rx_len;
  int64_t rx_mis;            // rx's address mod 16
  const int64_t* foff;
  const int32_t* flen;
  const int64_t* n_dev;
  int64_t ncap;
  const int32_t* f_seg;
  const int32_t* wslots;
  const int32_t* seg_state;
  const int64_t* bad;
  int64_t S;
};

ZK_DEV int64_t rs_frames(const RsBatch& b) {
  const int64_t nd = *b.n_dev;
  return nd < 0 ? 0 : (nd < b.ncap ? nd : b.ncap);
}

// 16 bytes of rx at p for the ring (p + rx_mis is a multiple of 16): one
// vector load where they lie inside rx, byte loads of the ones that do at
// rx's two ends, zeros past `end`.
ZK_DEV uint4 rs_fetch(const RsBatch& b, int64_t p, int64_t end) {
  uint4 v = {0u, 0u, 0u, 0u};
  if (p >= end) return v;
  if (p >= 0 && p + 16 <= b.rx_len)
    return *reinterpret_cast<const uint4*>(b.rx + p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (int i = 0; i < 16; ++i) {
    const int64_t q = p + i;
    if (q >= 0 && q < b.rx_len) w[i >> 2] |= (uint32_t)b.rx[q] << (8 * (i & 3));
  }
  v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
  return v;
}

// cnt[j] (FILL: read, else written): the paths frame j lists for a watcher.
template <bool FILL>
__global__ __launch_bounds__(RS_T) void rs_list_k(
    RsBatch b, int64_t* __restrict__ cnt, const int64_t* __restrict__ base,
    int64_t* __restrict__ ent, int32_t* __restrict__ elen, int64_t ecap,
    int64_t* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) uint32_t ring[RS_RING];
  const int lane = threadIdx.x;
  const int64_t j = blockIdx.x;
  // (everything up to the walk's end is wave-uniform)
  int32_t slot = RF_NONE;
  int64_t off = 0, L = 0;
  if (j < rs_frames(b)) {
    off = b.foff[j];
    L = b.flen[j];
    slot = resume_frame(b.rx, b.rx_len, off, L, b.bad, b.seg_state, b.wslots,
                        b.S, b.f_seg[j]);
  }
  int64_t room = 0, at = 0;
  if (FILL) {
    room = slot >= 0 ? cnt[j] : 0;
    if (room <= 0) return;
    at = base[j];
  } else if (slot == RF_NONE) {
    if (lane == 0) cnt[j] = 0;
    return;
  }
  const int64_t end = off + L;
  const int64_t c0 = ((off + RS_HEAD + b.rx_mis) & ~(int64_t)15) - b.rx_mis;
  const int64_t nch = (end - c0 + RS_CHUNK - 1) / RS_CHUNK;
  auto rd = [&](int64_t k) -> int32_t {
    const uint32_t r = (uint32_t)(k - c0);
    const uint32_t i = (r >> 2) & (RS_RING - 1);
    const uint64_t two = ((uint64_t)ring[(i + 1) & (RS_RING - 1)] << 32) |
                         ring[i];
    // (every lane read the same word: as a scalar the walk's state stays in
    // SGPRs and its branches are the scalar unit's)
    return __builtin_amdgcn_readfirstlane(
        (int32_t)bswap32((uint32_t)(two >> (8 * (r & 3)))));
  };
  auto emit = [&](int64_t m, int32_t g, int64_t po, int32_t pl) {
    if (!FILL) return;
    const int64_t x = at + m;
    if (m < room && x < ecap && (int)(m & (WAVE - 1)) == lane) {
      ent[x] = (int64_t)((uint64_t)g << 62) | po;
      elen[x] = pl;
    }
  };
  ResumeWalk w = resume_walk_begin(off);
  uint4 cur = rs_fetch(b, c0 + (int64_t)lane * 16, end);
  for (int64_t c = 0; c < nch; ++c) {
    // chunk c takes the place of chunk c - 2; the walk below never reads
    // before chunk c - 1 (it stopped at a word that reaches into chunk c)
    *reinterpret_cast<uint4*>(&ring[(c & 1) * (RS_CHUNK / 4) + lane * 4]) =
        cur;
    __syncthreads();
    if (c + 1 < nch)
      cur = rs_fetch(b, c0 + (c + 1) * RS_CHUNK + (int64_t)lane * 16, end);
    const int64_t got = c0 + (c + 1) * RS_CHUNK;
    resume_walk(w, got < end ? got : end, end, rd, emit);
    if (w.done) break;
    __syncthreads();
  }
  if (lane != 0) return;
  const int64_t m = w.done && w.ok ? w.m : 0;
  if (FILL) {
    // (m == room: the same walk over the same bytes)
    if (at + room > ecap) {
      const int64_t over = at + room - ecap;
      atomicAdd((unsigned long long*)&stats[RST_DROPPED],
                (unsigned long long)(over < room ? over : room));
    }
    return;
  }
  cnt[j] = slot >= 0 ? m : 0;
  if (m > 0)
    atomicAdd((unsigned long long*)&stats[slot >= 0 ? RST_LISTED
                                                    : RST_NO_SLOT],
              (unsigned long long)m);
}

// flag[e] (every e < ecap): entry e is an event; edec[e] = type | slot << 8.
__global__ __launch_bounds__(RD_T) void rs_decide_k(
    ZkTree t, RsBatch b, const int64_t* __restrict__ base,
    const int64_t* __restrict__ tot, const int64_t* __restrict__ ent,
    const int32_t* __restrict__ elen, int64_t ecap, int32_t* __restrict__ flag,
    int32_t* __restrict__ edec, int64_t* __restrict__ stats) {
  const int64_t e = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  const int64_t nd = tot[0];
  const int64_t ne = nd < 0 ? 0 : (nd < ecap ? nd : ecap);
  int32_t dec = 0;
  bool armed = false;
  if (e < ne) {
    const int64_t j = resume_entry_frame(base, rs_frames(b), e);
    const int64_t seg = j >= 0 ? b.f_seg[j] : -1;
    const int32_t slot = sess_in(seg, b.S) ? b.wslots[seg] : -1;
    const int64_t off = j >= 0 ? b.foff[j] : -1;
    const int64_t v = ent[e];
    const int32_t g = (int32_t)((uint64_t)v >> 62);
    const int64_t po = v & (((int64_t)1 << 62) - 1);
    const int32_t pl = elen[e];
    if (slot >= 0 && slot < 64 && off >= 0 && off + RS_HEAD <= b.rx_len &&
        pl >= 0 && po <= b.rx_len && pl <= b.rx_len - po) {
      const int64_t rel = ld_be64(b.rx + off + 8);
      const uint8_t* p = b.rx + po;
      const Found f = tree_lookup(t, p, pl);
      const bool there = f.node >= 0;
      const int32_t d = resume_decide(
          g, there, there ? ld_be64(t.store.slab + f.slot + 8) : 0,
          there ? t.pzxid[f.node] : 0, rel);
      if (d < 0) {
        wt_arm(t, p, pl, d == RD_ARM_CHILD ? WK_CHILD : WK_DATA, slot);
        armed = true;
      } else {
        dec = d | (slot << 8);
      }
    }
  }
  if (e < ecap) {
    flag[e] = dec != 0 ? 1 : 0;
    edec[e] = dec;
  }
  const uint64_t m = __ballot(armed);
  if (m != 0 && lane_id() == 0)
    atomicAdd((unsigned long long*)&stats[RST_REARMED],
              (unsigned long long)__popcll(m));
}

// pos: the exclusive scan of flag, tot[1] its sum.
__global__ __launch_bounds__(RD_T) void rs_emit_k(
    const int64_t* __restrict__ tot, const int64_t* __restrict__ ent,
    const int32_t* __restrict__ elen, int64_t ecap,
    const int32_t* __restrict__ flag, const int32_t* __restrict__ edec,
    const int64_t* __restrict__ pos, int32_t* __restrict__ ev_slot,
    int32_t* __restrict__ ev_type, int64_t* __restrict__ ev_poff,
    int32_t* __restrict__ ev_plen, int64_t* __restrict__ ev_total,
    int64_t* __restrict__ stats) {
  const int64_t e = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  if (e == 0) {
    const int64_t n = tot[1], wr = n < ecap ? n : ecap;
    ev_total[0] = stats[RST_WRITTEN] = wr;
    ev_total[1] = stats[RST_EVENTS] = n;
  }
  const int64_t nd = tot[0];
  const int64_t ne = nd < 0 ? 0 : (nd < ecap ? nd : ecap);
  if (e >= ne || flag[e] == 0) return;
  const int64_t x = pos[e];
  if (x < 0 || x >= ecap) return;                  // (never: the flags' sum)
  const int32_t dec = edec[e];
  ev_slot[x] = dec >> 8;
  ev_type[x] = dec & 0xff;
  ev_poff[x] = ent[e] & (((int64_t)1 << 62) - 1);
  ev_plen[x] = elen[e];
}

// The workspace's parts, in int64 words.
struct RsWork {
  int64_t cnt, base, tot, ent, pos, elen, flag, edec, scan, group, words;
};

static RsWork rs_work(int64_t ncap, int64_t ecap) {
  RsWork w;
  const int64_t half = (ecap + 1) / 2;             // int32 [ecap]
  int64_t o = 0;
  w.cnt = o; o += ncap;
  w.base = o; o += ncap;
  w.tot = o; o += 8;
  w.ent = o; o += ecap;
  w.pos = o; o += ecap;
  w.elen = o; o += half;
  w.flag = o; o += half;
  w.edec = o; o += half;
  w.scan = o; o += zk_scan_workspace(ncap > ecap ? ncap : ecap);
  w.group = o; o += zk_sess_group_workspace(ecap);
  w.words = o;
  return w;
}

}  // namespace zk

extern "C" {

// int64 words of zk_watch_resume_sessions' workspace (nothing in it needs
// zeroing).
int64_t zk_watch_resume_sessions_workspace(int64_t ncap, int64_t ecap) {
  return zk::rs_work(ncap > 0 ? ncap : 1, ecap > 0 ? ecap : 1).words;
}

// The catch-up of a session batch after its serve: frames foff / flen
// (*n_dev of them, at most ncap) of rx[0, rx_len) with the segment table g
// (its sessions are not read).  -> the events, ecap records of
// room, in stream order (ev_*; ev_total[0] written, [1] all), the same
// grouped by watcher slot (g_*, slot_first[65]: zk_sess_group_events), and
// stats[8]: events, events written, watches re-armed, paths listed, paths
// past the entry room (ecap), paths of live frames without a valid watcher
// slot.  ecap >= rx_len / 4 holds every list: a listed path takes at least
// its 4 length bytes.
int zk_watch_resume_sessions(
    const ZkTree* t, const uint8_t* rx, int64_t rx_len, const int64_t* foff,
    const int32_t* flen, const int64_t* n_dev, int64_t ncap, const ZkSegs* g,
    int64_t* ws, int64_t ecap, int32_t* ev_slot, int32_t* ev_type,
    int64_t* ev_poff, int32_t* ev_plen, int64_t* ev_total, int32_t* g_slot,
    int32_t* g_type, int64_t* g_poff, int32_t* g_plen, int64_t* slot_first,
    int64_t* stats, hipStream_t st) {
  if (t->wt_key == nullptr) return -1;
  if (ncap < 1 || ncap > 0x7fffffff || ecap < 1 || g == nullptr || g->S < 1 ||
      rx_len < 0)
    return (int)hipErrorInvalidValue;
  const zk::RsWork w = zk::rs_work(ncap, ecap);
  int64_t* cnt = ws + w.cnt;
  int64_t* base = ws + w.base;
  int64_t* tot = ws + w.tot;
  int64_t* ent = ws + w.ent;
  int64_t* pos = ws + w.pos;
  int32_t* elen = reinterpret_cast<int32_t*>(ws + w.elen);
  int32_t* flag = reinterpret_cast<int32_t*>(ws + w.flag);
  int32_t* edec = reinterpret_cast<int32_t*>(ws + w.edec);
  const zk::RsBatch b{rx, rx_len, (int64_t)((uintptr_t)rx & 15), foff, flen,
                      n_dev, ncap, g->f_seg, g->wslots, g->seg_state,
                      g->bad, g->S};
  if (hipMemsetAsync(stats, 0, zk::RST_N * sizeof(int64_t), st) != hipSuccess)
    return -4;
  zk::rs_list_k<false><<<(unsigned)ncap, zk::RS_T, 0, st>>>(
      b, cnt, nullptr, nullptr, nullptr, ecap, stats);
  ZK_LAUNCH_CHECK();
  int rc = zk_scan_excl_i64(cnt, base, ncap, tot, ws + w.scan, st);
  if (rc) return rc;
  zk::rs_list_k<true><<<(unsigned)ncap, zk::RS_T, 0, st>>>(
      b, cnt, base, ent, elen, ecap, stats);
  ZK_LAUNCH_CHECK();
  const unsigned nb = (unsigned)((ecap + zk::RD_T - 1) / zk::RD_T);
  zk::rs_decide_k<<<nb, zk::RD_T, 0, st>>>(*t, b, base, tot, ent, elen, ecap,
                                           flag, edec, stats);
  ZK_LAUNCH_CHECK();
  rc = zk_scan_excl_i32(flag, pos, ecap, tot + 1, ws + w.scan, st);
  if (rc) return rc;
  zk::rs_emit_k<<<nb, zk::RD_T, 0, st>>>(tot, ent, elen, ecap, flag, edec, pos,
                                         ev_slot, ev_type, ev_poff, ev_plen,
                                         ev_total, stats);
  ZK_LAUNCH_CHECK();
  return zk_sess_group_events(ev_slot, ev_type, ev_poff, ev_plen, ev_total,
                              ecap, ws + w.group, g_slot, g_type, g_poff,
                              g_plen, slot_first, st);
}

}  // extern "C"
