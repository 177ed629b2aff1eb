// The GPU tree's list path, GET_CHILDREN / GET_CHILDREN2 (the tree: zk_tree.h).
#include "zk_tree.h"
#include "zk_sess.h"

namespace zk {

// ---- list (GET_CHILDREN / GET_CHILDREN2) -------------------------------------
// The tree keeps no child links (they would put dependent memory trips on
// the create / delete / expiry paths).  Every live node carries its parent
// (node_parent) and its path word, so a batch of list requests is a join of
// "the parents somebody asked for" against one sweep of the node table —
// two sweeps a batch (sizes, then bytes), whatever the batch size:
//  1. list_mark_k, a thread per request: parse, look the path up, claim the
//     node in want[node] (atomicMin of the request index: the smallest index
//     asking for a parent is its leader, so the outcome does not depend on
//     scheduling); a watch=1 request that found its node arms the child
//     watch.  "/" has no node in this tree: NO_NODE, like every op on it.
//  2. list_sweep_k<false>, a thread per node: a live child of a claimed
//     parent adds 1 and 4 + name length to the leader's packed accumulator,
//     one atomic per wave per distinct parent (ballot loop);
//  3. list_size_k + the device-wide scan + list_total_k: frame sizes (an OK
//     reply past max_frame is demoted to a header-only SYSTEMERROR), the
//     smallest OK request of each parent becomes the writer of its strings,
//     offsets, the total against the output capacity;
//  4. list_head_k: headers, child counts and the GET_CHILDREN2 Stats;
//  5. list_sweep_k<true>: the same sweep; each child takes its bytes in the
//     writer's reply from the parent's cursor (one returning atomic per wave
//     per distinct parent + a wave prefix) and writes be32(len) + name.  The
//     order inside a reply is whatever the sweep gives, like ZooKeeper's;
//  6. list_copy_k, a wave per request: the other requests of a parent copy
//     the writer's string region; want[] goes back to the sentinel.
// No host read between the launches.
// MS (list_mark_sess_k): the list frames of a session batch of any op mix
// (GpuServer.serve_sessions_mixed).  A frame takes its watcher slot from its
// segment's row of the table M; a refused one (zk_sess.h sess_refusal) is
// answered header-only with the xid alone read: nothing is parsed, looked
// up, claimed in want[] or armed, and the later kernels see an error request
// (par -1), as a NO_NODE is.  Refusal is per lane and *M.bad grid-uniform.
constexpr int32_t LS_NONE = 0x7fffffff;        // want[] / writer idle
constexpr int LS_BYTES = 40;                   // acc: count << 40 | bytes
constexpr uint64_t LS_BMASK = (1ull << LS_BYTES) - 1;

struct ListWs {
  int64_t* ctr;                 // [8] 0: the stream overflowed the output
  int32_t* par;                 // [ncap] the node asked for (-1: none)
  int32_t* err;                 // [ncap]
  int32_t* xid;                 // [ncap]
  int32_t* op;                  // [ncap]
  int32_t* lead;                // [ncap] the parent's leader request
  int32_t* writer;              // [ncap] per leader: smallest OK request
  unsigned long long* acc;      // [ncap] per leader: children << 40 | bytes
  unsigned long long* cursor;   // [ncap] per leader: string bytes placed
  int64_t* sizes;               // [ncap] frame bytes
  int64_t* scan;                // zk_scan_workspace(ncap)
};

// (The kernels' parameters carry __restrict__; repeated on the inlined body
// it moved the plain instance's code, tools/kernel_resources.py --diff.)
template <bool MS>
ZK_DEV void list_mark_body(
    const ZkTree& t, const uint8_t* rx,
    const int64_t* foff, const int32_t* flen,
    const int64_t* n_dev, int64_t ncap, int32_t wslot,
    int32_t* want, const ListWs& w, const SegTable& M) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  w.acc[i] = 0;
  w.cursor[i] = 0;
  w.writer[i] = LS_NONE;
  w.lead[i] = LS_NONE;
  int32_t par = -1, err = ERR_OK, xid = 0, op = OP_PING;
  if (i < *n_dev) {
    int32_t ms_err = ERR_OK;           // MS: the segment's refusal
    if (MS) {
      const int64_t sg = M.f_seg[i];
      ms_err = sess_refusal(M.bad, M.seg_state, M.S, sg);
      if (ms_err == ERR_OK) wslot = M.wslots[sg];
    }
    if (MS && ms_err != ERR_OK) {
      xid = sess_xid(rx, foff[i], flen[i]);
      err = ms_err;
    } else {
      const ReqFields rq = parse_request(rx, foff[i], flen[i]);
      xid = rq.xid;
      op = rq.op;
      if (rq.status != ST_OK) {
        err = ERR_BAD_ARGUMENTS;
      } else if (op != OP_GET_CHILDREN && op != OP_GET_CHILDREN2) {
        err = ERR_UNIMPLEMENTED;
      } else {
        const uint8_t* p = rx + rq.poff;
        const int64_t node = tree_find(t, p, rq.pl);
        if (node < 0 || node >= t.store.cap) {
          err = ERR_NO_NODE;            // (no watch on a missing node)
        } else {
          par = (int32_t)node;
          atomicMin(&want[node], (int32_t)i);
          if (rq.arg == 1) wt_arm(t, p, rq.pl, WK_CHILD, wslot);
        }
      }
    }
  }
  w.par[i] = par;
  w.err[i] = err;
  w.xid[i] = xid;
  w.op[i] = op;
}

__global__ __launch_bounds__(TR_T) void list_mark_k(
    ZkTree t, const uint8_t* __restrict__ rx,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, int32_t wslot,
    int32_t* __restrict__ want, ListWs w) {
  list_mark_body<false>(t, rx, foff, flen, n_dev, ncap, wslot, want, w,
                        SegTable{});
}

__global__ __launch_bounds__(TR_T) void list_mark_sess_k(
    ZkTree t, const uint8_t* __restrict__ rx,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    int32_t* __restrict__ want, ListWs w, SegTable M) {
  list_mark_body<true>(t, rx, foff, flen, n_dev, ncap, -1, want, w, M);
}

// The sweep over the node table.  FILL = false: count; true: write.  Every
// lane stays in the ballot loop (its trip count is wave-uniform).
template <bool FILL>
__global__ __launch_bounds__(TR_T) void list_sweep_k(
    ZkTree t, const int32_t* __restrict__ want, ListWs w,
    const int64_t* __restrict__ rec_off, uint8_t* __restrict__ out) {
  if (FILL && w.ctr[0] != 0) return;               // (grid-uniform)
  const int64_t v = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t nn = min(t.counters[TC_NODES], t.store.cap);
  int32_t lead = LS_NONE, nl = 0;
  const uint8_t* name = nullptr;
  if (v < nn) {
    const int64_t p = t.node_parent[v];
    if (p >= 0 && p < t.store.cap) {
      lead = want[p];
      if (lead != LS_NONE) {
        const int64_t pw = t.node_pw[v];
        const int32_t skip = pw_len(t.node_pw[p]) + 1;
        nl = max(pw_len(pw) - skip, 0);
        name = node_path(t, pw) + skip;
      }
    }
  }
  bool active = lead != LS_NONE;
  // FILL: the parent's writer (none: every request of it failed or was
  // demoted) and the bytes its reply holds
  int32_t wr = LS_NONE;
  int64_t room = 0;
  if (FILL && active) {
    wr = w.writer[lead];
    room = (int64_t)(w.acc[lead] & LS_BMASK);
    active = wr != LS_NONE;
  }
  const int64_t sz = active ? 4 + (int64_t)nl : 0;
  const int lane = lane_id();
  uint64_t todo = __ballot(active);
  while (todo != 0) {
    const int first = __ffsll((unsigned long long)todo) - 1;
    const int32_t l0 = __shfl(lead, first, 64);
    const bool mine = active && lead == l0;
    const uint64_t m = __ballot(mine);
    // inclusive prefix of the group's sizes (lanes outside it carry 0)
    int64_t inc = mine ? sz : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t y = __shfl_up(inc, d, 64);
      if (lane >= d) inc += y;
    }
    const int64_t tot = __shfl(inc, 63, 64);
    if (!FILL) {
      if (lane == first)
        atomicAdd(&w.acc[l0],
                  ((unsigned long long)__popcll(m) << LS_BYTES) +
                      (unsigned long long)tot);
    } else {
      unsigned long long base = 0;
      if (lane == first)
        base = atomicAdd(&w.cursor[l0], (unsigned long long)tot);
      base = __shfl(base, first, 64);
      const int64_t pos = (int64_t)base + inc - sz;
      // (the count pass measured this reply: a child that does not fit it
      // means the tree changed under the batch; it is left out, in bounds)
      if (mine && pos + sz <= room) {
        uint8_t* d = out + rec_off[wr] + 24 + pos;
        st_be32(d, nl);
        copy_bytes(d + 4, name, nl);
      }
    }
    todo &= ~m;
  }
}

__global__ __launch_bounds__(TR_T) void list_size_k(
    const int32_t* __restrict__ want, const int64_t* __restrict__ n_dev,
    int64_t ncap, int64_t max_frame, ListWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  int64_t sz = 0;
  if (i < *n_dev) {
    sz = 4 + 16;
    const int32_t par = w.par[i];
    if (w.err[i] == ERR_OK && par >= 0) {
      const int32_t lead = want[par];
      w.lead[i] = lead;
      const int64_t full = sz + 4 + (int64_t)(w.acc[lead] & LS_BMASK) +
                           (w.op[i] == OP_GET_CHILDREN2 ? STAT_BYTES : 0);
      if (full > max_frame) {
        w.err[i] = ERR_SYSTEM;
      } else {
        sz = full;
        atomicMin(&w.writer[lead], (int32_t)i);
      }
    }
  }
  w.sizes[i] = sz;
}

// The stream total against the capacity (K13's convention: err 2 when it
// does not fit; then the total is 0 and nothing is written), the terminator.
__global__ void list_total_k(int64_t* __restrict__ total, int64_t out_cap,
                             int32_t* __restrict__ err, int32_t terminate,
                             uint8_t* __restrict__ out, ListWs w) {
  const int64_t T = *total;
  const bool over = T > out_cap;
  w.ctr[0] = over ? 1 : 0;
  *err = over ? 2 : 0;
  if (over) *total = 0;
  if (!over && terminate && T + 4 <= out_cap) st_be32(out + T, -1);
}

__global__ __launch_bounds__(TR_T) void list_head_k(
    ZkTree t, const int64_t* __restrict__ n_dev, int64_t ncap, ListWs w,
    const int64_t* __restrict__ rec_off, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap || i >= *n_dev || w.ctr[0] != 0) return;
  uint8_t* o = out + rec_off[i];
  const int32_t err = w.err[i];
  const int64_t sz = w.sizes[i];
  st_be32(o, (int32_t)(sz - 4));
  st_be32(o + 4, w.xid[i]);
  st_be64(o + 8, t.counters[TC_ZXID]);          // reads see the batch's base
  st_be32(o + 16, err);
  if (err != ERR_OK) return;
  const unsigned long long a = w.acc[w.lead[i]];
  st_be32(o + 20, (int32_t)(a >> LS_BYTES));
  if (w.op[i] == OP_GET_CHILDREN2)
    copy_bytes(o + 24 + (int64_t)(a & LS_BMASK),
               t.store.slab + t.store.slot_off[w.par[i]], STAT_BYTES);
}

// A wave per request: the string region of the parent's writer into every
// other OK reply of that parent; the claimed want[] words back to idle
// (every reader of them ran in an earlier launch).
__global__ __launch_bounds__(TR_T) void list_copy_k(
    const int64_t* __restrict__ n_dev, int64_t ncap,
    int32_t* __restrict__ want, ListWs w, const int64_t* __restrict__ rec_off,
    uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * (TR_T / 64) + (threadIdx.x >> 6);
  if (i >= ncap || i >= *n_dev) return;
  const int lane = lane_id();
  const int32_t par = w.par[i];
  if (par >= 0 && lane == 0) want[par] = LS_NONE;
  if (w.ctr[0] != 0 || par < 0 || w.err[i] != ERR_OK) return;
  const int32_t lead = w.lead[i];
  const int32_t wr = w.writer[lead];
  if (wr == (int32_t)i || wr == LS_NONE) return;
  const int64_t nb = (int64_t)(w.acc[lead] & LS_BMASK);
  const uint8_t* s = out + rec_off[wr] + 24;
  uint8_t* d = out + rec_off[i] + 24;
  const int64_t body = nb & ~(int64_t)15;
  for (int64_t k = (int64_t)lane * 16; k < body; k += 64 * 16) {
    uint4 x;
    __builtin_memcpy(&x, s + k, 16);
    __builtin_memcpy(d + k, &x, 16);
  }
  if (body + lane < nb) d[body + lane] = s[body + lane];
}

}  // namespace zk

extern "C" {

// Workspace of zk_tree_list for up to ncap requests (bytes; 16-aligned
// parts).  Nothing in it needs zeroing: list_mark_k resets what a batch
// reads.
static int64_t list_layout(int64_t ncap, uint8_t* ws, zk::ListWs* w) {
  auto a16 = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    uint8_t* p = ws != nullptr ? ws + o : nullptr;
    o += a16(bytes);
    return p;
  };
  uint8_t* ctr = take(64);
  uint8_t* i32s[6];
  for (auto& p : i32s) p = take(ncap * 4);
  uint8_t* acc = take(ncap * 8);
  uint8_t* cursor = take(ncap * 8);
  uint8_t* sizes = take(ncap * 8);
  uint8_t* scan = take(zk_scan_workspace(ncap > 0 ? ncap : 1) * 8);
  if (w != nullptr) {
    w->ctr = (int64_t*)ctr;
    w->par = (int32_t*)i32s[0];
    w->err = (int32_t*)i32s[1];
    w->xid = (int32_t*)i32s[2];
    w->op = (int32_t*)i32s[3];
    w->lead = (int32_t*)i32s[4];
    w->writer = (int32_t*)i32s[5];
    w->acc = (unsigned long long*)acc;
    w->cursor = (unsigned long long*)cursor;
    w->sizes = (int64_t*)sizes;
    w->scan = (int64_t*)scan;
  }
  return o;
}

int64_t zk_tree_list_workspace(int64_t ncap) {
  return list_layout(ncap > 0 ? ncap : 0, nullptr, nullptr);
}

// Answer a batch of GET_CHILDREN / GET_CHILDREN2 frames (foff / flen,
// *n_dev of them, at most ncap) from the tree: the framed replies in request
// order -> out[0, *total), their starts -> rec_off[ncap].  want: int32 per
// node slot of the tree, all LS_NONE (0x7fffffff) between calls (the kernels
// leave it so).  A reply frame longer than max_frame bytes (length word
// included) is answered SYSTEMERROR instead.  *err = 2 and *total = 0 when
// the stream does not fit out_cap.  See list_* above.
static int list_launch(const ZkTree* t, const uint8_t* rx,
                       const int64_t* foff, const int32_t* flen,
                       const int64_t* n_dev, int64_t ncap, int32_t wslot,
                       const zk::SegTable* M, int64_t max_frame,
                       int32_t* want, uint8_t* ws, int64_t ws_bytes,
                       uint8_t* out, int64_t out_cap, int64_t* rec_off,
                       int64_t* total, int32_t* err, int32_t terminate,
                       hipStream_t st) {
  if (out_cap < 0 || max_frame < 0) return -1;
  if (ncap <= 0) {
    if (hipMemsetAsync(total, 0, sizeof(int64_t), st) != hipSuccess) return -4;
    if (hipMemsetAsync(err, 0, sizeof(int32_t), st) != hipSuccess) return -4;
    if (terminate && out_cap >= 4 &&
        hipMemsetAsync(out, 0xFF, 4, st) != hipSuccess)
      return -4;
    return 0;
  }
  if (ncap >= zk::LS_NONE) return -1;              // request indices: int32
  if (ws_bytes < zk_tree_list_workspace(ncap) || ((uintptr_t)ws & 15))
    return -1;
  if (max_frame > zk::MAX_PACKET) max_frame = zk::MAX_PACKET;
  zk::ListWs w;
  list_layout(ncap, ws, &w);
  const unsigned nb = (unsigned)((ncap + zk::TR_T - 1) / zk::TR_T);
  const unsigned nbv = (unsigned)((t->store.cap + zk::TR_T - 1) / zk::TR_T);
  if (M != nullptr)
    zk::list_mark_sess_k<<<nb, zk::TR_T, 0, st>>>(*t, rx, foff, flen, n_dev,
                                                  ncap, want, w, *M);
  else
    zk::list_mark_k<<<nb, zk::TR_T, 0, st>>>(*t, rx, foff, flen, n_dev, ncap,
                                             wslot, want, w);
  ZK_LAUNCH_CHECK();
  if (nbv > 0) {
    zk::list_sweep_k<false><<<nbv, zk::TR_T, 0, st>>>(*t, want, w, rec_off,
                                                      out);
    ZK_LAUNCH_CHECK();
  }
  zk::list_size_k<<<nb, zk::TR_T, 0, st>>>(want, n_dev, ncap, max_frame, w);
  ZK_LAUNCH_CHECK();
  const int rc = zk_scan_excl_i64(w.sizes, rec_off, ncap, total, w.scan, st);
  if (rc) return rc;
  zk::list_total_k<<<1, 1, 0, st>>>(total, out_cap, err, terminate, out, w);
  ZK_LAUNCH_CHECK();
  zk::list_head_k<<<nb, zk::TR_T, 0, st>>>(*t, n_dev, ncap, w, rec_off, out);
  ZK_LAUNCH_CHECK();
  if (nbv > 0) {
    zk::list_sweep_k<true><<<nbv, zk::TR_T, 0, st>>>(*t, want, w, rec_off,
                                                     out);
    ZK_LAUNCH_CHECK();
  }
  const unsigned nbc =
      (unsigned)((ncap + zk::TR_T / 64 - 1) / (zk::TR_T / 64));
  zk::list_copy_k<<<nbc, zk::TR_T, 0, st>>>(n_dev, ncap, want, w, rec_off,
                                            out);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_tree_list(const ZkTree* t, const uint8_t* rx, const int64_t* foff,
                 const int32_t* flen, const int64_t* n_dev, int64_t ncap,
                 int32_t wslot, int64_t max_frame, int32_t* want, uint8_t* ws,
                 int64_t ws_bytes, uint8_t* out, int64_t out_cap,
                 int64_t* rec_off, int64_t* total, int32_t* err,
                 int32_t terminate, hipStream_t st) {
  return list_launch(t, rx, foff, flen, n_dev, ncap, wslot, nullptr,
                     max_frame, want, ws, ws_bytes, out, out_cap, rec_off,
                     total, err, terminate, st);
}

// zk_tree_list for the list frames of a session batch of any op mix: frame i
// is served for segment f_seg[i] (zk_sess_split_segments' table of the list
// class) — its watcher slot wslots[seg] arms a watch=1 list's child watch
// (outside 0..63: none) — or refused as zk_sess.h sess_refusal says
// (zk_sess_assign's seg_state / bad, S segments), header only.  g: the segment
// table; its sessions are not read.
int zk_tree_list_sessions(const ZkTree* t, const uint8_t* rx,
                          const int64_t* foff, const int32_t* flen,
                          const int64_t* n_dev, int64_t ncap, const ZkSegs* g,
                          int64_t max_frame, int32_t* want, uint8_t* ws,
                          int64_t ws_bytes, uint8_t* out, int64_t out_cap,
                          int64_t* rec_off, int64_t* total, int32_t* err,
                          int32_t terminate, hipStream_t st) {
  if (g == nullptr || g->f_seg == nullptr || g->wslots == nullptr ||
      g->seg_state == nullptr || g->bad == nullptr || g->S < 1)
    return -1;
  const zk::SegTable M{g->f_seg, g->wslots, g->seg_state, g->bad, g->S};
  return list_launch(t, rx, foff, flen, n_dev, ncap, -1, &M, max_frame, want,
                     ws, ws_bytes, out, out_cap, rec_off, total, err,
                     terminate, st);
}

}  // extern "C"
