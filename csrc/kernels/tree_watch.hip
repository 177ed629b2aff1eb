// The GPU tree's watch events: the masks a served batch (or a session expiry)
// fired expanded into notifications, the SET_WATCHES catch-up, and the watch
// table's maintenance: a closed session's bits dropped, the table rebuilt
// from the entries that still hold a watch (the table itself, wt_arm /
// wt_fire: zk_tree.h).
#include "zk_tree.h"

namespace zk {

// ---- watch event expansion ------------------------------------------------
// Notifications of a served batch, in request order (ZooKeeper delivers a
// session's notifications in zxid order; write i of a batch has zxid base +
// i + 1): request i contributes one event per watcher bit of the masks it
// fired — m_path (type by op), m_path_child (NodeDeleted, a watcher holding
// both a data and a child watch on a deleted path is told once), m_parent
// (NodeChildrenChanged on the parent).  Three launches: counts + block
// sums, one-block scan of the sums, write.
ZK_DEV bool wt_live(const int32_t* r_op, const int32_t* r_err, int64_t i) {
  const int32_t op = r_op[i];
  return r_err[i] == ERR_OK &&
         (op == OP_SET_DATA || op == OP_CREATE || op == OP_DELETE);
}

ZK_DEV int64_t wt_count(const int32_t* r_op, const int32_t* r_err,
                        const int64_t* fired, int64_t i, bool in) {
  if (!in || !wt_live(r_op, r_err, i)) return 0;
  const int64_t* f = fired + (int64_t)WT_REC * i;
  return __popcll((uint64_t)f[0]) + __popcll((uint64_t)f[1]) +
         __popcll((uint64_t)f[2]);
}

__global__ __launch_bounds__(TR_T) void wt_count_k(
    const int32_t* __restrict__ r_op, const int32_t* __restrict__ r_err,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int64_t* __restrict__ fired, int64_t* __restrict__ bsum) {
  __shared__ int64_t sm[TR_T / 64 + 1];
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const bool in = i < ncap && i < *n_dev;
  int64_t tot;
  block_excl_scan(wt_count(r_op, r_err, fired, i, in), sm, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

ZK_DEV void wt_emit(uint64_t m, int32_t type, int64_t pw, int64_t& o,
                    int64_t cap, int32_t* ev_slot, int32_t* ev_type,
                    int64_t* ev_poff, int32_t* ev_plen) {
  while (m) {
    const int b = __builtin_ctzll(m);
    m &= m - 1;
    if (o < cap) {
      ev_slot[o] = b;
      ev_type[o] = type;
      ev_poff[o] = pw >> 24;
      ev_plen[o] = pw_len(pw);
    }
    ++o;
  }
}

__global__ __launch_bounds__(TR_T) void wt_expand_k(
    const int32_t* __restrict__ r_op, const int32_t* __restrict__ r_err,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int64_t* __restrict__ fired, const int64_t* __restrict__ bsum,
    int64_t nb, int64_t cap, int32_t* __restrict__ ev_slot,
    int32_t* __restrict__ ev_type, int64_t* __restrict__ ev_poff,
    int32_t* __restrict__ ev_plen, int64_t* __restrict__ ev_total) {
  __shared__ int64_t sm[TR_T / 64 + 1];
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const bool in = i < ncap && i < *n_dev;
  const int64_t c = wt_count(r_op, r_err, fired, i, in);
  int64_t tot;
  int64_t o = bsum[blockIdx.x] + block_excl_scan(c, sm, &tot);
  if (blockIdx.x == nb - 1 && threadIdx.x == 0) {
    const int64_t all = bsum[blockIdx.x] + tot;
    ev_total[0] = min(all, cap);     // events written (the encoder's count)
    ev_total[1] = all;               // events fired (> [0]: overflow)
  }
  if (c == 0) return;
  const int64_t* f = fired + (int64_t)WT_REC * i;
  const int32_t op = r_op[i];
  const int32_t t0 = op == OP_SET_DATA ? NT_DATA_CHANGED
                   : op == OP_CREATE ? NT_CREATED : NT_DELETED;
  wt_emit((uint64_t)f[0], t0, f[3], o, cap, ev_slot, ev_type, ev_poff,
          ev_plen);
  wt_emit((uint64_t)f[1], NT_DELETED, f[3], o, cap, ev_slot, ev_type,
          ev_poff, ev_plen);
  wt_emit((uint64_t)f[2], NT_CHILDREN_CHANGED, f[4], o, cap, ev_slot,
          ev_type, ev_poff, ev_plen);
}

// ---- SET_WATCHES catch-up (one workgroup) ---------------------------------
// A resumed session re-sends its watches with relZxid = the last zxid it saw
// (lib/zk-session.js:421-471, lib/zk-buffer.js:255-273).  For every path
// (SURVEY Appendix D): data watch — node gone: NodeDeleted, mzxid > rel:
// NodeDataChanged, else re-armed; exist watch — node there: NodeCreated,
// else re-armed; child watch — node gone: NodeDeleted, pzxid > rel:
// NodeChildrenChanged, else re-armed.  Events name the request's path
// bytes (offsets into rx), in request order (data, exist, child lists).
constexpr int WR_T = 1024;

__global__ __launch_bounds__(WR_T) void wt_resume_k(
    ZkTree t, const uint8_t* __restrict__ rx,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, int32_t wslot,
    int64_t* __restrict__ ent, int64_t ent_cap, int64_t cap,
    int32_t* __restrict__ ev_type, int64_t* __restrict__ ev_poff,
    int32_t* __restrict__ ev_plen, int64_t* __restrict__ out) {
  __shared__ int64_t sm[WR_T / 64 + 1];
  __shared__ int64_t s_n, s_rel, s_drop;
  int64_t o = 0, rearmed = 0;
  if (threadIdx.x == 0) s_drop = 0;
  const int64_t nfr = min(*n_dev, ncap);
  for (int64_t fr = 0; fr < nfr; ++fr) {
    // thread 0 lists the frame's paths (kind << 62 | off << 24 | len);
    // a frame that is not a well-formed SET_WATCHES lists none
    if (threadIdx.x == 0) {
      const ReqFields rq = parse_request(rx, foff[fr], flen[fr]);
      int64_t m = 0;
      // (a count or a length that runs past the frame ends the listing: a
      // listed path takes at least its 4 length bytes of the frame, so
      // ent_cap = stream bytes / 4 holds every frame's list)
      if (rq.status == ST_OK && rq.op == OP_SET_WATCHES) {
        const int64_t end = foff[fr] + flen[fr];
        int64_t k = rq.voff;
        for (int g = 0; g < 3 && k + 4 <= end; ++g) {
          const int32_t c = max(ld_be32(rx + k), 0);
          k += 4;
          for (int32_t j = 0; j < c && k + 4 <= end; ++j) {
            const int32_t l = max(ld_be32(rx + k), 0);
            if (k + 4 + l > end) {
              k = end;
              break;
            }
            if (m < ent_cap)
              ent[m] = ((int64_t)g << 62) | ((k + 4) << 24) | l;
            ++m;
            k += 4 + l;
          }
        }
      }
      s_n = min(m, ent_cap);
      s_drop += m - s_n;
      s_rel = rq.rel;
    }
    __syncthreads();
    const int64_t n = s_n, rel = s_rel;
    for (int64_t b = 0; b < n; b += WR_T) {
      const int64_t j = b + threadIdx.x;
      int32_t type = 0;
      int64_t po = 0;
      int32_t pl = 0;
      if (j < n) {
        const int64_t e = ent[j];
        const int g = (int)((uint64_t)e >> 62);
        po = (e >> 24) & ((1ll << 38) - 1);
        pl = (int32_t)(e & 0xFFFFFF);
        const uint8_t* p = rx + po;
        const Found f = tree_lookup(t, p, pl);
        if (g == 0) {                              // data watch
          if (f.node < 0) type = NT_DELETED;
          else if (ld_be64(t.store.slab + f.slot + 8) > rel)
            type = NT_DATA_CHANGED;
        } else if (g == 1) {                       // exist watch
          if (f.node >= 0) type = NT_CREATED;
        } else {                                   // child watch
          if (f.node < 0) type = NT_DELETED;
          else if (t.pzxid[f.node] > rel) type = NT_CHILDREN_CHANGED;
        }
        if (type == 0) {
          wt_arm(t, p, pl, g == 2 ? WK_CHILD : WK_DATA, wslot);
          ++rearmed;
        }
      }
      int64_t tot;
      const int64_t x = o + block_excl_scan(type != 0 ? 1 : 0, sm, &tot);
      if (type != 0 && x < cap) {
        ev_type[x] = type;
        ev_poff[x] = po;
        ev_plen[x] = pl;
      }
      o += tot;
    }
    __syncthreads();
  }
  int64_t tot;
  block_excl_scan(rearmed, sm, &tot);
  if (threadIdx.x == 0) {
    out[0] = min(o, cap);        // events written
    out[1] = tot;                // watches re-armed
    out[2] = o;                  // events (> out[0]: overflow)
    out[3] = s_drop;             // listed paths that found no room in ent
  }
}

// ---- maintenance ------------------------------------------------------------
// A closed session's watches go with it: clear watcher slot wslot's bit from
// every mask (the entries stay; zk_watch_rebuild drops the empty ones).
__global__ __launch_bounds__(TR_T) void wt_drop_k(ZkTree t, int32_t wslot) {
  const unsigned long long keep = ~(1ull << wslot);
  const int64_t n = 2 * (t.wt_hmask + 1);
  for (int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * TR_T)
    if (t.wt_mask[i] & ~keep) t.wt_mask[i] &= keep;
}

// Entries are never removed by a fire, so every path ever watched keeps one:
// the rebuild inserts the old table's entries that still hold a watch into
// the tree's new (zeroed) table by their two hash words; the counters move
// with them.  Entries that find no room (a smaller table) are counted lost.
__global__ __launch_bounds__(TR_T) void wt_rebuild_k(
    ZkTree t, const int64_t* __restrict__ okey,
    const int64_t* __restrict__ omask, int64_t ohmask) {
  const int64_t on = ohmask + 1;
  unsigned long long* stat = &t.wt_mask[2 * (t.wt_hmask + 1)];
  for (int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x; i < on;
       i += (int64_t)gridDim.x * TR_T) {
    if (i < WT_STATS && omask[2 * on + i] != 0)
      atomicAdd(&stat[i], (unsigned long long)omask[2 * on + i]);
    const int64_t k = okey[2 * i], g = okey[2 * i + 1];
    const int64_t m0 = omask[2 * i], m1 = omask[2 * i + 1];
    if (k == 0 || g == 0 || (m0 | m1) == 0) continue;
    const int64_t s = wt_slot(t, (uint64_t)k, (uint64_t)g, true);
    if (s < 0) {
      atomicAdd(&stat[WS_LOST], (unsigned long long)(__popcll(m0) +
                                                    __popcll(m1)));
      continue;
    }
    t.wt_mask[2 * s] = (unsigned long long)m0;
    t.wt_mask[2 * s + 1] = (unsigned long long)m1;
  }
}

}  // namespace zk

extern "C" {

// Expand the watch masks a served batch fired (tree_serve's `fired`) into
// notification events in request order: ev_slot (watcher slot), ev_type,
// ev_poff / ev_plen (path in the tree's path arena); ev_total[0] = events
// written (at most `cap`), ev_total[1] = events fired.  bsum: ceil(ncap /
// 256) int64.
int zk_watch_events(const int32_t* r_op, const int32_t* r_err,
                    const int64_t* n_dev, int64_t ncap, const int64_t* fired,
                    int64_t* bsum, int64_t cap, int32_t* ev_slot,
                    int32_t* ev_type, int64_t* ev_poff, int32_t* ev_plen,
                    int64_t* ev_total, hipStream_t st) {
  if (ncap <= 0) return hipMemsetAsync(ev_total, 0, 16, st);
  const int64_t nb = (ncap + zk::TR_T - 1) / zk::TR_T;
  zk::wt_count_k<<<(unsigned)nb, zk::TR_T, 0, st>>>(r_op, r_err, n_dev, ncap,
                                                    fired, bsum);
  ZK_LAUNCH_CHECK();
  const int rc = zk::bscan_launch(bsum, nb, st);
  if (rc) return rc;
  zk::wt_expand_k<<<(unsigned)nb, zk::TR_T, 0, st>>>(
      r_op, r_err, n_dev, ncap, fired, bsum, nb, cap, ev_slot, ev_type,
      ev_poff, ev_plen, ev_total);
  ZK_LAUNCH_CHECK();
  return 0;
}

// SET_WATCHES catch-up for the frames (foff / flen, *n_dev of them) of a
// resumed session with watcher slot wslot: events (ev_type, ev_poff /
// ev_plen into rx) for what changed after each frame's relZxid, the other
// watches re-armed.  out[0] = events written (<= cap), out[1] = re-armed
// watches, out[2] = events, out[3] = listed paths past ent_cap (neither
// answered nor re-armed).  ent: scratch for ent_cap paths; the stream's
// bytes / 4 hold any frame's list.
int zk_watch_resume(const ZkTree* t, const uint8_t* rx, const int64_t* foff,
                    const int32_t* flen, const int64_t* n_dev, int64_t ncap,
                    int32_t wslot, int64_t* ent, int64_t ent_cap, int64_t cap,
                    int32_t* ev_type, int64_t* ev_poff, int32_t* ev_plen,
                    int64_t* out, hipStream_t st) {
  if (t->wt_key == nullptr) return -1;
  zk::wt_resume_k<<<1, zk::WR_T, 0, st>>>(*t, rx, foff, flen, n_dev, ncap,
                                           wslot, ent, ent_cap, cap, ev_type,
                                           ev_poff, ev_plen, out);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_watch_drop(const ZkTree* t, int32_t wslot, hipStream_t st) {
  if (t->wt_key == nullptr || wslot < 0 || wslot > 63) return -1;
  const int64_t n = 2 * (t->wt_hmask + 1);
  const int64_t nb = (n + zk::TR_T - 1) / zk::TR_T;
  zk::wt_drop_k<<<(unsigned)(nb < 1024 ? nb : 1024), zk::TR_T, 0, st>>>(
      *t, wslot);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_watch_rebuild(const ZkTree* t, const int64_t* okey,
                     const int64_t* omask, int64_t ohmask, hipStream_t st) {
  if (t->wt_key == nullptr || okey == t->wt_key) return -1;
  const int64_t nb = (ohmask + zk::TR_T) / zk::TR_T;
  zk::wt_rebuild_k<<<(unsigned)(nb < 1024 ? nb : 1024), zk::TR_T, 0, st>>>(
      *t, okey, omask, ohmask);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
