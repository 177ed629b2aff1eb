// Session batches: one request stream carries the whole frames of S
// connections, concatenated, with a per-segment table of sessions and
// watcher slots (the rule: zk_sess.h).  The passes around the serve (whose
// MS instances, tree.hip, read what these write):
//   sess_assign_k      a lane per frame: its segment, the torn frames counted
//   sess_first_k       a lane per boundary: each segment's first frame, the
//                      table's order, and whether its session is alive
//   sess_ranges_k      after the reply (and notification) encode: every
//                      connection's slice of the reply stream, every
//                      watcher's slice of the notification stream
//   sess_split_seg_k   a batch of any op mix, after the split by engine class
//                      (tree_mix.hip): a lane per frame carries its segment
//                      to its place beside the class's compacted frame table
//   sess_ev_hist_k,    the batch's watch events grouped by watcher slot,
//   sess_ev_scatter_k  stable (request order inside a slot), in route.hip's
//                      shape: a per-block histogram, the device-wide scan of
//                      the counts in slot-major order, a scatter whose ranks
//                      come from wave ballots and an LDS prefix over the
//                      block's waves.  No lane waits for another and no
//                      counter is shared.
#include "zk_tree.h"
#include "zk_sess.h"
#include "zk_mix.h"
#include "zk_session.h"

namespace zk {

constexpr int SE_T = 256;
constexpr int SE_SLOTS = 64;          // watcher slots of a server

// bad[0]: torn frames + the table's own faults; bad[1]: the smallest segment
// one was found in, as an unsigned minimum (all ones: none).
ZK_DEV void sess_count_bad(int64_t* __restrict__ bad, int32_t mine,
                           int64_t seg) {
  const uint64_t m = __ballot(mine != 0);
  if (m == 0) return;                              // (wave-uniform)
  int64_t tot = mine, lo = mine ? seg : INT64_MAX;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    tot += __shfl_xor(tot, d, 64);
    const int64_t o = __shfl_xor(lo, d, 64);
    lo = o < lo ? o : lo;
  }
  if (lane_id() == 0) {
    atomicAdd((unsigned long long*)&bad[0], (unsigned long long)tot);
    atomicMin((unsigned long long*)&bad[1], (unsigned long long)lo);
  }
}

__global__ __launch_bounds__(SE_T) void sess_assign_k(
    const int64_t* __restrict__ off, const int32_t* __restrict__ len,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int64_t* __restrict__ starts, int64_t S,
    int32_t* __restrict__ f_seg, int64_t* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * SE_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < ncap ? nd : ncap;
  int32_t torn = 0;
  int64_t seg = 0;
  if (j < nf && j >= 0) {
    const int64_t o = off[j];
    seg = sess_seg(starts, S, o - 4);
    torn = sess_torn(starts, S, seg, o + (int64_t)len[j]) ? 1 : 0;
    f_seg[j] = (int32_t)seg;
    if (seg < 0) seg = 0;
  }
  sess_count_bad(bad, torn, seg);
}

__global__ __launch_bounds__(SE_T) void sess_first_k(
    const int64_t* __restrict__ off, const int64_t* __restrict__ n_dev,
    int64_t ncap, const int64_t* __restrict__ starts,
    const int64_t* __restrict__ sessions, int64_t S,
    int64_t* __restrict__ first, int32_t* __restrict__ seg_state,
    int64_t* __restrict__ bad, ZkSessionTable tab, int32_t has_tab,
    int64_t server_id) {
  const int64_t s = (int64_t)blockIdx.x * SE_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  int32_t mine = 0;
  if (s <= S) {
    first[s] = sess_first(off, nf, starts[s]);
    mine = sess_boundary_bad(starts, S, s);
    if (s < S) {
      int32_t st = 0;
      const int64_t sid = sessions[s];
      if (has_tab && sid != 0 && sid != SESS_DEV) {
        const int64_t idx = sess_slot(tab, sid, server_id);
        const bool alive = idx >= 0 && tab.sid[idx] == sid &&
                           tab.state[idx] == SS_ALIVE;
        st = alive ? 0 : 1;
      }
      seg_state[s] = st;
    }
  }
  sess_count_bad(bad, mine, s);
}

// rep_off[s] = the reply stream's offset of segment s's first frame, s in
// 0..S (the stream total where it has none after it); all 0 when the encoder
// refused the stream (err bit 1).  With slot_first: likewise slot_off[0..64]
// of the grouped notification stream.
__global__ __launch_bounds__(SE_T) void sess_ranges_k(
    const int64_t* __restrict__ first, int64_t S,
    const int64_t* __restrict__ rec_off, const int64_t* __restrict__ n_dev,
    int64_t ncap, const int64_t* __restrict__ total,
    const int32_t* __restrict__ err, int64_t* __restrict__ rep_off,
    const int64_t* __restrict__ slot_first,
    const int64_t* __restrict__ ev_rec_off,
    const int64_t* __restrict__ ev_count, int64_t ecap,
    const int64_t* __restrict__ ev_bytes, const int32_t* __restrict__ ev_err,
    int64_t* __restrict__ slot_off) {
  const int64_t s = (int64_t)blockIdx.x * SE_T + threadIdx.x;
  if (s <= S) {
    const int64_t nd = *n_dev;
    const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
    const int64_t f = first[s];
    int64_t o = 0;
    if (!(*err & 2)) o = f >= 0 && f < nf ? rec_off[f] : *total;
    rep_off[s] = o;
  }
  if (slot_first != nullptr && s <= SE_SLOTS) {
    const int64_t nd = *ev_count;
    const int64_t ne = nd < 0 ? 0 : (nd < ecap ? nd : ecap);
    const int64_t f = slot_first[s];
    int64_t o = 0;
    if (!(*ev_err & 2)) o = f >= 0 && f < ne ? ev_rec_off[f] : *ev_bytes;
    slot_off[s] = o;
  }
}

// f_seg_c[cls[i]][sub[i]] = f_seg[i] for the batch's frames (the split's cls /
// sub, tree_mix.hip): the class tables c0 / c1 / c2, ncap entries each.  A row
// the split's outputs do not bear out (sess_split_at) writes nothing.
static_assert(MIX_CLASSES == 3, "sess_split_at: three class tables");
__global__ __launch_bounds__(SE_T) void sess_split_seg_k(
    const int32_t* __restrict__ f_seg, const int32_t* __restrict__ cls,
    const int32_t* __restrict__ sub, const int64_t* __restrict__ n_dev,
    int64_t ncap, int32_t* __restrict__ c0, int32_t* __restrict__ c1,
    int32_t* __restrict__ c2) {
  const int64_t i = (int64_t)blockIdx.x * SE_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < ncap ? nd : ncap;
  if (i < 0 || i >= nf) return;
  const int32_t c = cls[i];
  const int64_t j = sub[i];
  if (sess_split_at(c, j, ncap) < 0) return;
  int32_t* d = c == 0 ? c0 : c == 1 ? c1 : c2;
  d[j] = f_seg[i];
}

// ---- event grouping ----------------------------------------------------------
ZK_DEV int32_t sess_ev_slot(const int32_t* __restrict__ ev_slot, int64_t i,
                            int64_t ne) {
  return i < ne ? (int32_t)((uint32_t)ev_slot[i] & (SE_SLOTS - 1)) : -1;
}

ZK_DEV int64_t sess_ev_count(const int64_t* __restrict__ ev_total,
                             int64_t ecap) {
  const int64_t nd = ev_total[0];
  return nd < 0 ? 0 : (nd < ecap ? nd : ecap);
}

// hist[slot * blocks + block]: the block's events of the slot.
__global__ __launch_bounds__(SE_T) void sess_ev_hist_k(
    const int32_t* __restrict__ ev_slot, const int64_t* __restrict__ ev_total,
    int64_t ecap, int64_t* __restrict__ hist) {
  __shared__ int32_t h[SE_SLOTS];
  if (threadIdx.x < SE_SLOTS) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * SE_T + threadIdx.x;
  const int32_t o = sess_ev_slot(ev_slot, i, sess_ev_count(ev_total, ecap));
  if (o >= 0) atomicAdd(&h[o], 1);
  __syncthreads();
  if (threadIdx.x < SE_SLOTS)
    hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// base: the exclusive scan of hist (slot-major), *total its sum.
__global__ __launch_bounds__(SE_T) void sess_ev_scatter_k(
    const int32_t* __restrict__ ev_slot, const int32_t* __restrict__ ev_type,
    const int64_t* __restrict__ ev_poff, const int32_t* __restrict__ ev_plen,
    const int64_t* __restrict__ ev_total, int64_t ecap,
    const int64_t* __restrict__ base, const int64_t* __restrict__ total,
    int32_t* __restrict__ g_slot, int32_t* __restrict__ g_type,
    int64_t* __restrict__ g_poff, int32_t* __restrict__ g_plen,
    int64_t* __restrict__ slot_first) {
  __shared__ int32_t cnt[SE_T / WAVE][SE_SLOTS];
  const int64_t i = (int64_t)blockIdx.x * SE_T + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x <= SE_SLOTS)
    slot_first[threadIdx.x] =
        threadIdx.x < SE_SLOTS ? base[(int64_t)threadIdx.x * gridDim.x]
                               : *total;
  const int64_t ne = sess_ev_count(ev_total, ecap);
  // a workgroup past the written events has nothing to rank (the grid covers
  // ecap; block-uniform, before the barrier)
  if ((int64_t)blockIdx.x * SE_T >= ne) return;
  const int32_t o = sess_ev_slot(ev_slot, i, ne);
  // (lane 63's mask: 1 << 63 is taken unsigned)
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  int32_t r = 0;
  for (int32_t w = 0; w < SE_SLOTS; ++w) {
    const uint64_t m = __ballot(o == w);
    if (o == w) r = __popcll(m & below);
    if (lane == 0) cnt[wv][w] = __popcll(m);
  }
  __syncthreads();
  if (o < 0) return;
  for (int k = 0; k < wv; ++k) r += cnt[k][o];
  const int64_t pos = base[(int64_t)o * gridDim.x + blockIdx.x] + r;
  if (pos < 0 || pos >= ecap) return;              // (never: the counts' sum)
  g_slot[pos] = o;
  g_type[pos] = ev_type[i];
  g_poff[pos] = ev_poff[i];
  g_plen[pos] = ev_plen[i];
}

static int64_t ev_blocks(int64_t ecap) { return (ecap + SE_T - 1) / SE_T; }

}  // namespace zk

extern "C" {

// The segments of a batch (zk_sess.h): frames off / len (*n_dev of them, at
// most ncap), the table starts[S + 1] / sessions[S] -> f_seg[ncap] (written
// for the batch's frames), first[S + 1], seg_state[S] (0 serve, 1 the
// session is not alive in `tab`; tab null: every segment is served) and
// bad[2] (the count, the first bad segment or -1).
int zk_sess_assign(const int64_t* off, const int32_t* len,
                   const int64_t* n_dev, int64_t ncap, const int64_t* starts,
                   const int64_t* sessions, int64_t S,
                   const ZkSessionTable* tab, int64_t server_id,
                   int32_t* f_seg, int64_t* first, int32_t* seg_state,
                   int64_t* bad, hipStream_t st) {
  if (S < 1 || ncap < 0) return (int)hipErrorInvalidValue;
  if (hipMemsetAsync(bad, 0, 8, st) != hipSuccess) return -4;
  if (hipMemsetAsync(bad + 1, 0xFF, 8, st) != hipSuccess) return -4;
  if (ncap > 0) {
    zk::sess_assign_k<<<(unsigned)((ncap + zk::SE_T - 1) / zk::SE_T),
                        zk::SE_T, 0, st>>>(off, len, n_dev, ncap, starts, S,
                                           f_seg, bad);
    ZK_LAUNCH_CHECK();
  }
  zk::sess_first_k<<<(unsigned)((S + 1 + zk::SE_T - 1) / zk::SE_T), zk::SE_T,
                     0, st>>>(off, n_dev, ncap, starts, sessions, S, first,
                              seg_state, bad,
                              tab != nullptr ? *tab : ZkSessionTable{},
                              tab != nullptr ? 1 : 0, server_id);
  ZK_LAUNCH_CHECK();
  return 0;
}

// After the reply encode (rec_off, *total, *err) and, with slot_first, the
// grouped notification encode (ev_rec_off over *ev_count <= ecap records,
// *ev_bytes, *ev_err): rep_off[S + 1] and slot_off[65].
int zk_sess_ranges(const int64_t* first, int64_t S, const int64_t* rec_off,
                   const int64_t* n_dev, int64_t ncap, const int64_t* total,
                   const int32_t* err, int64_t* rep_off,
                   const int64_t* slot_first, const int64_t* ev_rec_off,
                   const int64_t* ev_count, int64_t ecap,
                   const int64_t* ev_bytes, const int32_t* ev_err,
                   int64_t* slot_off, hipStream_t st) {
  if (S < 1) return (int)hipErrorInvalidValue;
  const int64_t n = S + 1 > zk::SE_SLOTS + 1 ? S + 1 : zk::SE_SLOTS + 1;
  zk::sess_ranges_k<<<(unsigned)((n + zk::SE_T - 1) / zk::SE_T), zk::SE_T, 0,
                      st>>>(first, S, rec_off, n_dev, ncap, total, err,
                            rep_off, slot_first, ev_rec_off, ev_count, ecap,
                            ev_bytes, ev_err, slot_off);
  ZK_LAUNCH_CHECK();
  return 0;
}

// After zk_sess_assign (f_seg) and zk_tree_mix_split (cls / sub) of one frame
// table (*n_dev frames, at most ncap): every frame's segment beside its
// class's compacted frame table, f_seg_c0 / c1 / c2 [ncap] (written for the
// class's frames).  One launch, no host read.
int zk_sess_split_segments(const int32_t* f_seg, const int32_t* cls,
                           const int32_t* sub, const int64_t* n_dev,
                           int64_t ncap, int32_t* f_seg_c0, int32_t* f_seg_c1,
                           int32_t* f_seg_c2, hipStream_t st) {
  if (ncap < 0) return (int)hipErrorInvalidValue;
  if (ncap == 0) return 0;
  zk::sess_split_seg_k<<<(unsigned)((ncap + zk::SE_T - 1) / zk::SE_T),
                         zk::SE_T, 0, st>>>(f_seg, cls, sub, n_dev, ncap,
                                            f_seg_c0, f_seg_c1, f_seg_c2);
  ZK_LAUNCH_CHECK();
  return 0;
}

// int64 words of zk_sess_group_events' workspace for ecap events.
int64_t zk_sess_group_workspace(int64_t ecap) {
  const int64_t nh = zk::SE_SLOTS * zk::ev_blocks(ecap > 0 ? ecap : 1);
  return 2 * nh + 8 + zk_scan_workspace(nh);
}

// The ev_total[0] (<= ecap) written events of a batch (zk_watch_events'
// records) -> the same records in slot-major order, request order inside a
// slot (g_*), and slot_first[65]: slot w's records are [slot_first[w],
// slot_first[w + 1]).
int zk_sess_group_events(const int32_t* ev_slot, const int32_t* ev_type,
                         const int64_t* ev_poff, const int32_t* ev_plen,
                         const int64_t* ev_total, int64_t ecap, int64_t* ws,
                         int32_t* g_slot, int32_t* g_type, int64_t* g_poff,
                         int32_t* g_plen, int64_t* slot_first,
                         hipStream_t st) {
  if (ecap <= 0) return (int)hipErrorInvalidValue;
  const int64_t nb = zk::ev_blocks(ecap);
  const int64_t nh = zk::SE_SLOTS * nb;
  int64_t* hist = ws;
  int64_t* base = ws + nh;
  int64_t* total = ws + 2 * nh;
  zk::sess_ev_hist_k<<<(unsigned)nb, zk::SE_T, 0, st>>>(ev_slot, ev_total,
                                                        ecap, hist);
  ZK_LAUNCH_CHECK();
  const int rc = zk_scan_excl_i64(hist, base, nh, total, ws + 2 * nh + 8, st);
  if (rc) return rc;
  zk::sess_ev_scatter_k<<<(unsigned)nb, zk::SE_T, 0, st>>>(
      ev_slot, ev_type, ev_poff, ev_plen, ev_total, ecap, base, total, g_slot,
      g_type, g_poff, g_plen, slot_first);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
