// Close and expire many sessions in one pass (GpuServer.close_sessions, and
// serve_sessions / serve_sessions_mixed with close=True; the rules:
// zk_close.h).  zk_tree_expire ends one session with one sweep of the node
// table and one finish; K sessions that end between two launches cost K of
// each.  Here the K sessions' ephemerals go in one sweep, each session as its
// own closeSession txn (session rank k of the list: zxid base + k + 1), the
// watches the removals fire are recorded as tree_expire_wt_k records them, the
// closing sessions' own watches are dropped first and the session table's
// entries die.  The passes:
//   cl_frames_k   (a session batch) a lane per frame: close_frame; a closing
//                 frame marks its segment and turns its own reply's err from
//                 UNIMPLEMENTED into OK (the serve has written the row; the
//                 reply is the same 20 bytes, so a presized encode stands)
//   (the device-wide scan of the segments' marks: segment order is stream
//   order, no counter is shared and no lane waits)
//   cl_gather_k   a lane per segment: (session, watcher slot) of closing
//                 segment number k to place k of the list
//   cl_set_k      a lane per listed session: its id into the set, its watcher
//                 slot's bit into the drop mask
//   cl_drop_k     one sweep of the watch table: the drop mask's bits cleared
//                 from both masks of every entry (wt_drop_k for a mask)
//   cl_mark_k     one coalesced sweep of eph[]: cmark[v] = rank + 1 of a node
//                 whose owner is in the set, else 0 — so the removal's "has
//                 this entry an eraser in this launch" is one load, as eph is
//                 in tree_expire_k, not a probe chain on its dependent path
//   cl_remove_k   a lane per marked node: tree_expire_body's removal with the
//                 rank's zxid, one tombstone tag for the launch and removed[]
//                 counted per session
//   (tree_finish_k: the zxid moves by the device count K, the frees publish)
//   cl_table_k    a lane per listed id: the session table's entry closes
// No host read: every grid is sized from a capacity and every loop is bounded
// by a device count clipped to it.
#include "zk_tree.h"
#include "zk_close.h"
#include "zk_session.h"

namespace zk {

constexpr int CL_T = 256;

// stats[]: what GpuServer.close_stats reports (with the events' own totals)
enum : int { CST_FRAMES = 0, CST_SESSIONS = 1, CST_REMOVED = 2, CST_N = 8 };

// the scalars in the workspace (tot[])
enum : int { CT_K = 0, CT_DROP = 1, CT_N = 8 };

// The workspace's parts, in int64 words.  rec comes first: the caller reads
// the records (zk_watch_events) from the workspace's head.
struct ClWork {
  int64_t rec, tot, closing, pos, sid, wslot, key, rank, cmark, scan, words;
  int64_t set_cap;
};

static ClWork cl_work(int64_t cap_frames, int64_t S, int64_t node_cap) {
  ClWork w;
  int64_t o = 0;
  w.set_cap = close_set_cap(S);
  w.rec = o; o += 8 + (int64_t)WT_REC * cap_frames;
  w.tot = o; o += CT_N;
  w.closing = o; o += (S + 1) / 2;                 // int32 [S]
  w.pos = o; o += S;
  w.sid = o; o += S;
  w.wslot = o; o += (S + 1) / 2;                   // int32 [S]
  w.key = o; o += w.set_cap;
  w.rank = o; o += (w.set_cap + 1) / 2;            // int32 [set_cap]
  w.cmark = o; o += (node_cap + 1) / 2;            // int32 [node_cap]
  w.scan = o; o += zk_scan_workspace(S);
  w.words = o;
  return w;
}

// The list as the passes after the frames read it: K sessions (a device
// count clipped to the room, or the host's), their ids and watcher slots.
struct ClList {
  const int64_t* k_dev;      // null: k_host
  int64_t k_host, kcap;
  const int64_t* sid;
  const int32_t* wslot;      // null: none has a watcher slot
};

ZK_DEV int64_t cl_count(const ClList& l) {
  const int64_t k = l.k_dev != nullptr ? *l.k_dev : l.k_host;
  return k < 0 ? 0 : (k < l.kcap ? k : l.kcap);
}

// The set's writes on the device: lanes insert concurrently.
struct CloseDevOps {
  ZK_DEV int64_t cas(int64_t* p, int64_t expect, int64_t want) const {
    return (int64_t)atomicCAS((unsigned long long*)p,
                              (unsigned long long)expect,
                              (unsigned long long)want);
  }
  ZK_DEV void amin(int32_t* p, int32_t v) const { atomicMin(p, v); }
};

__global__ __launch_bounds__(CL_T) void cl_frames_k(
    const uint8_t* __restrict__ rx, int64_t rx_len,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int32_t* __restrict__ f_seg, const int32_t* __restrict__ seg_state,
    const int64_t* __restrict__ bad, int64_t S, int32_t* __restrict__ r_err,
    int32_t* __restrict__ closing, int64_t* __restrict__ stats) {
  const int64_t j = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  bool cl = false;
  if (j < nf) {
    const int64_t seg = f_seg[j];
    // (only a reply the serve left UNIMPLEMENTED: one it refused for a reason
    // of its own — an ordered batch's rank overflow — stays refused)
    cl = close_frame(rx, rx_len, foff[j], flen[j], bad, seg_state, S, seg) &&
         r_err[j] == ERR_UNIMPLEMENTED;
    if (cl) {
      closing[seg] = 1;
      r_err[j] = ERR_OK;
    }
  }
  const uint64_t m = __ballot(cl);
  if (m != 0 && lane_id() == 0)
    atomicAdd((unsigned long long*)&stats[CST_FRAMES],
              (unsigned long long)__popcll(m));
}

// pos: the exclusive scan of closing.
__global__ __launch_bounds__(CL_T) void cl_gather_k(
    ZkTree t, const int32_t* __restrict__ closing,
    const int64_t* __restrict__ pos, const int64_t* __restrict__ sessions,
    const int32_t* __restrict__ wslots, int64_t S, int64_t* __restrict__ sid,
    int32_t* __restrict__ wslot) {
  const int64_t s = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  if (s >= S || closing[s] == 0) return;
  const int64_t k = pos[s];
  if (k < 0 || k >= S) return;                     // (never: the marks' sum)
  sid[k] = sess_of(t, sessions[s]);
  wslot[k] = wslots[s];
}

__global__ __launch_bounds__(CL_T) void cl_set_k(
    ClList l, int64_t* __restrict__ key, int32_t* __restrict__ rank,
    int64_t set_cap, int64_t* __restrict__ tot, int64_t* __restrict__ stats) {
  const int64_t k = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  const int64_t K = cl_count(l);
  if (k == 0) stats[CST_SESSIONS] = K;
  uint64_t bit = 0;
  if (k < K) {
    close_set_insert(key, rank, set_cap, l.sid[k], (int32_t)k, CloseDevOps{});
    if (l.wslot != nullptr) bit = close_drop_mask(l.wslot[k]);
  }
  // the wave's bits in one atomic
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) bit |= __shfl_xor(bit, d, 64);
  if (bit != 0 && lane_id() == 0)
    atomicOr((unsigned long long*)&tot[CT_DROP], (unsigned long long)bit);
}

__global__ __launch_bounds__(CL_T) void cl_drop_k(
    ZkTree t, const int64_t* __restrict__ tot) {
  const unsigned long long drop = (unsigned long long)tot[CT_DROP];
  if (drop == 0) return;
  const int64_t n = 2 * (t.wt_hmask + 1);
  for (int64_t i = (int64_t)blockIdx.x * CL_T + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * CL_T)
    if (t.wt_mask[i] & drop) t.wt_mask[i] &= ~drop;
}

// cmark[v] for every v < ncap (nothing of it needs zeroing between calls).
__global__ __launch_bounds__(CL_T) void cl_mark_k(
    ZkTree t, ClList l, int64_t ncap, const int64_t* __restrict__ key,
    const int32_t* __restrict__ rank, int64_t set_cap,
    int32_t* __restrict__ cmark) {
  const int64_t v = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  if (v >= ncap || cl_count(l) == 0) return;       // (the removal returns too)
  const int64_t owner = v < t.counters[TC_NODES] ? t.eph[v] : 0;
  cmark[v] = owner != 0 ? close_set_find(key, rank, set_cap, owner) + 1 : 0;
}

// tree_expire_body (tree.hip) for the marked nodes: see there for why the
// loads are issued together, why the owner comes from a contiguous shadow and
// why the instance with the watch fire is a kernel of its own.  What differs:
// the removal of session rank k carries zxid base + k + 1 (every closeSession
// is a txn of its own; the parent's pzxid takes the max), the launch has one
// tombstone tag (the shift tells the holes of this launch, whichever session
// made them), removed[k] is counted per session, and the fired masks lose the
// drop mask's bits (a bit armed while the drop sweep ran cannot reach a
// closing watcher).
template <bool WT>
ZK_DEV void cl_remove_body(
    const ZkTree& t, const ClList& l, int64_t ncap,
    int32_t* __restrict__ cmark, unsigned long long* __restrict__ removed,
    const int64_t* __restrict__ tot, int64_t* __restrict__ rec,
    int64_t rec_cap, int64_t* __restrict__ stats) {
  const int64_t K = cl_count(l);
  if (K == 0) return;                              // (uniform: cmark unwritten)
  const int64_t v = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  const int32_t mk = v < ncap ? cmark[v] : 0;
  int32_t rk = mk - 1;
  bool hit = mk > 0 && rk < K;
  const int64_t base = t.counters[TC_ZXID];
  const int64_t zx = base + rk + 1;
  const int64_t tag = tomb_tag(base + 1);
  int64_t par = -1;
  int32_t dflag = 1;
  if (hit) {
    const int64_t poff = t.node_path_off[v];
    const int32_t plen = t.node_path_len[v];
    const int64_t p0 = t.node_parent[v];
    if (p0 >= 0)
      dflag = __hip_atomic_load(&t.dirty[p0], __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
    const int64_t es = tree_erase_slot(t, v, t.path_arena + poff, plen, tag);
    hit = es >= 0;
    if (hit) {
      // entries of the closing sessions are never moved (their erasers may be
      // probing for them): marked nodes block, as `session`'s do in ht_shift
      ht_shift_if(t, es, tag,
                  [&](int64_t node) { return cmark[node] == 0; });
      par = p0;
      if (par >= 0) parent_touch(t, par, -1, true, zx);
      t.eph[v] = 0;
      if (WT) {
        const uint64_t keep = ~(uint64_t)tot[CT_DROP];
        const int64_t ws = wt_find(t, t.path_arena + poff, plen);
        const uint64_t m0 = wt_fire_at(t, ws, WK_DATA) & keep;
        const uint64_t m1 = wt_fire_at(t, ws, WK_CHILD) & keep & ~m0;
        const int64_t ppw = par >= 0 ? t.node_pw[par] : 0;
        const uint64_t m2 =
            par >= 0 ? wt_fire(t, node_path(t, ppw), pw_len(ppw), WK_CHILD) &
                           keep
                     : 0;
        if ((m0 | m1 | m2) != 0 && rec != nullptr) {
          const int64_t k = (int64_t)atomicAdd((unsigned long long*)&rec[0],
                                               1ull);
          if (k < rec_cap) {
            int64_t* f = rec + 8 + (int64_t)WT_REC * k;
            f[0] = (int64_t)m0;
            f[1] = (int64_t)m1;
            f[2] = (int64_t)m2;
            f[3] = pw_pack(poff, plen);
            f[4] = ppw;
          }
        }
      }
    }
    // (after the erase: a live val with a mark is an entry whose eraser is
    // still to come)
    cmark[v] = 0;
  }
  // removed[] per session: a round per distinct rank among the wave's
  // removals (wave-uniform), one atomic each
  uint64_t todo = __ballot(hit);
  while (todo != 0) {
    const int lead = __builtin_ctzll(todo);
    const int32_t r = __shfl(rk, lead, 64);
    const uint64_t m = __ballot(hit && rk == r);
    if (lane_id() == lead)
      atomicAdd(&removed[r], (unsigned long long)__popcll(m));
    todo &= ~m;
  }
  // the frees' ticket also counts the total
  wave_free(t, hit ? v : -1,
            reinterpret_cast<unsigned long long*>(&stats[CST_REMOVED]));
  wave_mark_dirty_at(t, par, dflag);
}

__global__ __launch_bounds__(CL_T) void cl_remove_k(
    ZkTree t, ClList l, int64_t ncap, int32_t* __restrict__ cmark,
    unsigned long long* __restrict__ removed, const int64_t* __restrict__ tot,
    int64_t* __restrict__ stats) {
  cl_remove_body<false>(t, l, ncap, cmark, removed, tot, nullptr, 0, stats);
}

__global__ __launch_bounds__(CL_T) void cl_remove_wt_k(
    ZkTree t, ClList l, int64_t ncap, int32_t* __restrict__ cmark,
    unsigned long long* __restrict__ removed, const int64_t* __restrict__ tot,
    int64_t* __restrict__ rec, int64_t rec_cap, int64_t* __restrict__ stats) {
  cl_remove_body<true>(t, l, ncap, cmark, removed, tot, rec, rec_cap, stats);
}

// session_close_k's rule (session.hip) for the list.
__global__ __launch_bounds__(CL_T) void cl_table_k(ClList l,
                                                   ZkSessionTable tab,
                                                   int64_t server_id) {
  const int64_t k = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  if (k >= cl_count(l)) return;
  const int64_t s = l.sid[k];
  const int64_t idx = sess_slot(tab, s, server_id);
  if (idx >= 0 && tab.sid[idx] == s) tab.state[idx] = SS_CLOSED;
}

static_assert(CL_T == TR_T, "block_ticket's default block size");

static unsigned cl_blocks(int64_t n) {
  return (unsigned)((n + CL_T - 1) / CL_T);
}

}  // namespace zk

extern "C" {

// int64 words of the close passes' workspace for a server of cap_frames
// frames a batch, lists of up to S sessions (a session batch's segment count)
// and a tree of node_cap node slots.  Nothing in it needs zeroing.  Its head
// is the record area of the watches the removals fire: [0] records wanted,
// [8 + 5 k) record k < cap_frames (zk_tree_expire's rec).
int64_t zk_close_workspace(int64_t cap_frames, int64_t S, int64_t node_cap) {
  return zk::cl_work(cap_frames > 0 ? cap_frames : 0, S > 0 ? S : 1,
                     node_cap > 0 ? node_cap : 0).words;
}

// Pass 1 of a session batch, after its serve and before its reply encode:
// frames foff / flen (*n_dev of them, at most ncap) of rx[0, rx_len) with
// the segment table g.  Every CLOSE_SESSION frame of a live segment of a sound table
// (close_frame) whose reply the serve left UNIMPLEMENTED is answered OK
// (r_err) and closes its segment; the closing segments' (session, watcher
// slot), in segment order, become the workspace's list and their number its
// device count, for zk_close_sessions with sids null.  stats[8] is zeroed;
// [0] counts the closing frames.
int zk_close_frames(const ZkTree* t, const uint8_t* rx, int64_t rx_len,
                    const int64_t* foff, const int32_t* flen,
                    const int64_t* n_dev, int64_t ncap, const ZkSegs* g,
                    int32_t* r_err, int64_t cap_frames, int64_t node_cap,
                    int64_t* ws, int64_t* stats, hipStream_t st) {
  if (g == nullptr) return (int)hipErrorInvalidValue;
  const int64_t S = g->S;
  if (S < 1 || S > 0x7fffffff || ncap < 0 || rx_len < 0 || cap_frames < 0 ||
      node_cap < 0)
    return (int)hipErrorInvalidValue;
  const zk::ClWork w = zk::cl_work(cap_frames, S, node_cap);
  int32_t* closing = reinterpret_cast<int32_t*>(ws + w.closing);
  if (hipMemsetAsync(stats, 0, zk::CST_N * sizeof(int64_t), st) != hipSuccess ||
      hipMemsetAsync(closing, 0, (size_t)S * sizeof(int32_t), st) != hipSuccess)
    return -4;
  if (ncap > 0) {
    zk::cl_frames_k<<<zk::cl_blocks(ncap), zk::CL_T, 0, st>>>(
        rx, rx_len, foff, flen, n_dev, ncap, g->f_seg, g->seg_state, g->bad, S,
        r_err, closing, stats);
    ZK_LAUNCH_CHECK();
  }
  const int rc = zk_scan_excl_i32(closing, ws + w.pos, S, ws + w.tot + zk::CT_K,
                                  ws + w.scan, st);
  if (rc) return rc;
  zk::cl_gather_k<<<zk::cl_blocks(S), zk::CL_T, 0, st>>>(
      *t, closing, ws + w.pos, g->sessions, g->wslots, S, ws + w.sid,
      reinterpret_cast<int32_t*>(ws + w.wslot));
  ZK_LAUNCH_CHECK();
  return 0;
}

// Passes 2-7: end the listed sessions.  sids[K] / wslots[K] (wslots may be
// null), K <= S; or sids null: the list zk_close_frames left in the workspace
// (K on the device).  Session rank k's ephemerals are removed with zxid base +
// k + 1 and counted in removed[k] (accumulated; room for K, without sids for
// S), the zxid counter moves by K, the freed nodes are published.  On a tree with a watch table
// the listed watcher slots' bits are dropped from every mask first and the
// watches the removals fire are recorded at the workspace's head (at most
// cap_frames records; [0] counts the wanted).  tab (may be null): the listed
// ids' entries of the session table close.  stats[8]: [1] = K, [2] += nodes
// removed ([0] is zk_close_frames'; the direct form zeroes all).  The
// workspace is zk_close_workspace(cap_frames, S, node_cap), node_cap = the
// tree's node slots.
int zk_close_sessions(const ZkTree* t, const int64_t* sids,
                      const int32_t* wslots, int64_t K, int64_t S,
                      int64_t cap_frames, int64_t node_cap,
                      const ZkSessionTable* tab, int64_t server_id,
                      int64_t* ws, unsigned long long* removed, int64_t* stats,
                      hipStream_t st) {
  // (node_cap is the tree's: the shift looks up the mark of any indexed node)
  if (S < 1 || S > 0x7fffffff || cap_frames < 0 ||
      node_cap != t->store.cap || (sids != nullptr && (K < 0 || K > S)))
    return (int)hipErrorInvalidValue;
  const zk::ClWork w = zk::cl_work(cap_frames, S, node_cap);
  int64_t* tot = ws + w.tot;
  int64_t* key = ws + w.key;
  int32_t* rank = reinterpret_cast<int32_t*>(ws + w.rank);
  int32_t* cmark = reinterpret_cast<int32_t*>(ws + w.cmark);
  int64_t* rec = ws + w.rec;
  zk::ClList l;
  if (sids != nullptr) {
    l = zk::ClList{nullptr, K, S, sids, wslots};
    if (hipMemsetAsync(stats, 0, zk::CST_N * sizeof(int64_t), st) != hipSuccess)
      return -4;
  } else {
    l = zk::ClList{tot + zk::CT_K, 0, S, ws + w.sid,
                   reinterpret_cast<const int32_t*>(ws + w.wslot)};
  }
  if (hipMemsetAsync(tot + zk::CT_DROP, 0, 8, st) != hipSuccess ||
      hipMemsetAsync(rec, 0, 8, st) != hipSuccess ||
      hipMemsetAsync(key, 0, (size_t)w.set_cap * 8, st) != hipSuccess ||
      hipMemsetAsync(rank, 0x7f, (size_t)w.set_cap * 4, st) != hipSuccess)
    return -4;
  zk::cl_set_k<<<zk::cl_blocks(S), zk::CL_T, 0, st>>>(l, key, rank, w.set_cap,
                                                     tot, stats);
  ZK_LAUNCH_CHECK();
  const bool wt = t->wt_key != nullptr;
  if (wt) {
    const int64_t n = 2 * (t->wt_hmask + 1);
    const int64_t nb = (n + zk::CL_T - 1) / zk::CL_T;
    zk::cl_drop_k<<<(unsigned)(nb < 1024 ? nb : 1024), zk::CL_T, 0, st>>>(*t,
                                                                         tot);
    ZK_LAUNCH_CHECK();
  }
  if (node_cap > 0) {
    const unsigned nb = zk::cl_blocks(node_cap);
    zk::cl_mark_k<<<nb, zk::CL_T, 0, st>>>(*t, l, node_cap, key, rank,
                                           w.set_cap, cmark);
    ZK_LAUNCH_CHECK();
    if (wt)
      zk::cl_remove_wt_k<<<nb, zk::CL_T, 0, st>>>(
          *t, l, node_cap, cmark, removed, tot, rec, cap_frames, stats);
    else
      zk::cl_remove_k<<<nb, zk::CL_T, 0, st>>>(*t, l, node_cap, cmark, removed,
                                               tot, stats);
    ZK_LAUNCH_CHECK();
  }
  const int rc = zk::finish_launch(t, l.k_dev, l.k_host, 1, st);
  if (rc) return rc;
  if (tab != nullptr) {
    zk::cl_table_k<<<zk::cl_blocks(S), zk::CL_T, 0, st>>>(l, *tab, server_id);
    ZK_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
