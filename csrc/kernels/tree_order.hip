// The GPU tree's in-batch ordering pass and the ordered serve over it (the
// tree: zk_tree.h; the serve kernel: tree.hip, through serve_launch).
#include "zk_tree.h"
#include "zk_order_clip.h"

namespace zk {

// ---- in-batch ordering (tree_order_*) ---------------------------------------
// ZooKeeper applies a session's pipelined requests in order.  Two requests
// of a batch conflict when they touch the same path and one writes it, or
// when one creates / deletes a CHILD of the path the other operates on (the
// child write changes the parent's cversion / numChildren / pzxid and needs
// the parent to exist; a parent delete needs it gone):
//   * every request with a path joins its own path's group as an A member;
//   * a CREATE / DELETE also joins its parent's group as a C member (a
//     SEQUENTIAL create only that one: its own name is fresh).
// Edges inside a group (the later request runs in a later pass): A-A when
// the group has an A writer, A-C and C-A always, C-C never (children of one
// parent commute).  rank[i] = the longest chain of edges ending at i,
// computed by relaxation (`passes` + 1 rounds; a rank >= passes is refused
// with SYSTEMERROR, as before).  A scratch hash table groups the batch by
// path hash (a 64-bit collision merges two groups: extra ordering, never
// less); only ordered groups get member lists (offsets from a block scan of
// the group sizes: no shared counter).  No kernel here puts more than one
// atomic per block on a shared word, except the per-group counters (a
// single word sustains ~88 returning atomics per us, MI355X_MICROARCH.md).
constexpr int64_t ORD_MAX_GROUP = 1 << 16;   // larger ordered groups: refused
constexpr int ORD_F = 21;                     // bits per packed group count
constexpr int64_t ORD_FM = (1ll << ORD_F) - 1;

struct OrderWs {
  int64_t* ctr;      // [4] -, max rank, scratch top, -
  int64_t* key;      // [h] path hash | 1
  int64_t* cnt;      // [h] A | A writers << 21 | C << 42
  int32_t* fill;     // [h] member-list fill
  int32_t* lastw;    // [h] 1 + index of the group's last writer (A or C)
  int32_t* base;     // [h] member-list offset within its block of entries
  int64_t* bsum;     // [h / TR_T] block totals, then exclusive offsets
  int64_t* eidx;     // [2 ncap] request -> own (A) entry, parent (C) entry
  int32_t* members;  // [2 ncap] request << 1 | (1 = C member)
  int32_t* rnk;      // [ncap] relaxed ranks
  int64_t mask;      // h - 1
};

ZK_DEV bool ord_has_path(int32_t op) {
  return op == OP_CREATE || op == OP_DELETE || op == OP_SET_DATA ||
         op == OP_GET_DATA || op == OP_EXISTS || op == OP_GET_CHILDREN ||
         op == OP_GET_CHILDREN2 || op == OP_GET_ACL || op == OP_SYNC;
}

ZK_DEV bool ord_writes(int32_t op) {
  return op == OP_CREATE || op == OP_DELETE || op == OP_SET_DATA;
}

ZK_DEV int64_t ord_na(int64_t c) { return c & ORD_FM; }
ZK_DEV int64_t ord_naw(int64_t c) { return (c >> ORD_F) & ORD_FM; }
ZK_DEV int64_t ord_nc(int64_t c) { return (c >> (2 * ORD_F)) & ORD_FM; }
ZK_DEV int64_t ord_size(int64_t c) { return ord_na(c) + ord_nc(c); }

// a group with at least one edge
ZK_DEV bool ord_grouped(int64_t c) {
  return (ord_naw(c) >= 1 && ord_na(c) >= 2) ||
         (ord_na(c) >= 1 && ord_nc(c) >= 1);
}

ZK_DEV int64_t ord_entry(const OrderWs& w, int64_t key) {
  int64_t sl = key & w.mask;
  for (int64_t probe = 0; probe <= w.mask; ++probe) {
    const int64_t k = (int64_t)atomicCAS((unsigned long long*)&w.key[sl],
                                         0ull, (unsigned long long)key);
    if (k == 0 || k == key) return sl;
    sl = (sl + 1) & w.mask;
  }
  return -1;
}

__global__ __launch_bounds__(TR_T) void ord_insert_k(
    const uint8_t* __restrict__ rx, ZkReqOut q,
    const int64_t* __restrict__ n_dev, int64_t ncap, OrderWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  int64_t ea = -1, ec = -1;
  if (i < *n_dev && q.status[i] == ST_OK && ord_has_path(q.opcode[i])) {
    const int32_t op = q.opcode[i];
    const uint8_t* p = rx + q.path_off[i];
    const int32_t pl = q.path_len[i];
    const bool wr = ord_writes(op);
    const bool seq = op == OP_CREATE && (q.arg[i] & CF_SEQUENTIAL);
    if (!seq) {
      ea = ord_entry(w, (int64_t)(path_hash(p, pl) | 1ull));
      if (ea >= 0) {
        atomicAdd((unsigned long long*)&w.cnt[ea],
                  1ull + (wr ? 1ull << ORD_F : 0ull));
        if (wr) atomicMax(&w.lastw[ea], (int32_t)i + 1);
      }
    }
    if (op == OP_CREATE || op == OP_DELETE) {
      int32_t cut = pl - 1;
      while (cut > 0 && p[cut] != '/') --cut;
      if (cut > 0) {                   // the root's children: no group
        ec = ord_entry(w, (int64_t)(path_hash(p, cut) | 1ull));
        if (ec >= 0) {
          atomicAdd((unsigned long long*)&w.cnt[ec], 1ull << (2 * ORD_F));
          atomicMax(&w.lastw[ec], (int32_t)i + 1);
        }
      }
    }
  }
  w.eidx[2 * i] = ea;
  w.eidx[2 * i + 1] = ec;
}

// member-list offsets: a block scan of the ordered groups' sizes per TR_T
// entries
__global__ __launch_bounds__(TR_T) void ord_base_k(OrderWs w) {
  __shared__ int64_t sm[TR_T / 64 + 1];
  const int64_t e = (int64_t)blockIdx.x * TR_T + threadIdx.x;  // h % TR_T == 0
  const int64_t cw = w.cnt[e];
  const int64_t c = ord_grouped(cw) ? ord_size(cw) : 0;
  int64_t tot;
  const int64_t x = block_excl_scan(c, sm, &tot);
  if (c) w.base[e] = (int32_t)x;
  if (threadIdx.x == 0) w.bsum[blockIdx.x] = tot;
}

// exclusive scan of the block totals in place (one block)
constexpr int ORD_SCAN_T = 1024;
__global__ __launch_bounds__(ORD_SCAN_T) void ord_bscan_k(int64_t* bsum,
                                                          int64_t nbh) {
  __shared__ int64_t sm[ORD_SCAN_T / 64 + 1];
  const int64_t per = (nbh + ORD_SCAN_T - 1) / ORD_SCAN_T;
  const int64_t b0 = (int64_t)threadIdx.x * per;
  const int64_t b1 = min(b0 + per, nbh);
  int64_t sum = 0;
  for (int64_t k = b0; k < b1; ++k) sum += bsum[k];
  int64_t tot;
  int64_t x = block_excl_scan(sum, sm, &tot);
  for (int64_t k = b0; k < b1; ++k) {
    const int64_t v = bsum[k];
    bsum[k] = x;
    x += v;
  }
}

ZK_DEV int32_t* ord_list(const OrderWs& w, int64_t e) {
  return w.members + w.bsum[e / TR_T] + w.base[e];
}

__global__ __launch_bounds__(TR_T) void ord_fill_k(int64_t ncap, OrderWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  w.rnk[i] = 0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t e = w.eidx[2 * i + c];
    if (e < 0 || !ord_grouped(w.cnt[e])) continue;
    const int32_t pos = atomicAdd(&w.fill[e], 1);
    ord_list(w, e)[pos] = ((int32_t)i << 1) | c;
  }
}

// One relaxation round: rank[i] = 1 + the largest rank of an earlier
// request it has an edge to (in place: a rank never exceeds its chain).
__global__ __launch_bounds__(TR_T) void ord_relax_k(int64_t ncap, OrderWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  int32_t r = 0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t e = w.eidx[2 * i + c];
    if (e < 0) continue;
    const int64_t cw = w.cnt[e];
    if (!ord_grouped(cw)) continue;
    const int64_t sz = ord_size(cw);
    if (sz > ORD_MAX_GROUP) { r = ORD_RANK; break; }   // refused wholesale
    const bool aw = ord_naw(cw) >= 1;
    const int32_t* m = ord_list(w, e);
    // earlier A members with an edge to i form a chain among themselves
    // (A-A edges need an A writer, and then every A pair has one), earlier
    // C members do not: their count + 1 is a lower bound of the rank that
    // makes a one-path group exact in the first round
    int32_t na = 0, anyc = 0;
    for (int64_t k = 0; k < sz; ++k) {
      const int32_t x = m[k];
      const int32_t j = x >> 1;
      if (j >= (int32_t)i) continue;
      const bool jc = x & 1;
      const bool edge = c == 0 ? (jc || aw) : !jc;
      if (!edge) continue;
      r = max(r, w.rnk[j] + 1);
      if (jc) anyc = 1;
      else ++na;
    }
    r = max(r, (c == 0 && aw ? na : min(na, 1)) + anyc);
  }
  w.rnk[i] = min(r, (int32_t)ORD_RANK);
}

__global__ __launch_bounds__(TR_T) void ord_rank_k(int64_t ncap, OrderWs w,
                                                   uint8_t* __restrict__ rank) {
  __shared__ int32_t smx[TR_T / 64];
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  int32_t r = 0;
  bool later_write = false;
  if (i < ncap) {
    r = w.rnk[i];
    // a read of the path whose own group is written later in the batch (by
    // a writer of the path or a child create / delete) snapshots its reply
    const int64_t e = w.eidx[2 * i];
    later_write = e >= 0 && ord_grouped(w.cnt[e]) &&
                  w.lastw[e] > (int32_t)i + 1;
    rank[i] = (uint8_t)(r | (later_write ? ORD_SNAP : 0));
  }
  // the batch's largest rank: one atomic per block
  int32_t mx = r;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
  if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < TR_T / 64; ++k) mx = max(mx, smx[k]);
    if (mx > 0) atomicMax((unsigned long long*)&w.ctr[1],
                          (unsigned long long)mx);
  }
}

// ---- deferral instead of refusal (ord_clip_*; the rules: zk_order_clip.h) ----
// A session batch of any op mix behind a socket: a frame of the serve's class
// whose rank the passes cannot reach, and everything after it in its
// connection, leaves the batch before the first serve pass (its segment
// becomes -1: every engine, the catch-up and the close pass refuse a frame of
// no segment without effect) and stays pending with its connection.  Removing
// requests only lowers the ranks of the rest (a rank is a longest chain over
// earlier requests), so the rank bytes stay valid upper bounds and no
// surviving frame has a rank >= passes.  All tables here are the WHOLE
// batch's (cls / sub: the split's; f_seg: the assign's), nall its device
// frame count; every index is checked against ncap and S.
// (the kernels' own name for the launchers' ZkOrdClip, zk_abi.h)
struct OrdClip : ZkOrdClip {};

__global__ __launch_bounds__(TR_T) void ord_clip_init_k(OrdClip c,
                                                        int64_t ncap) {
  const int64_t s = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (s < c.S) c.clipf[s] = ncap;
  if (s == 0) *c.deferred = 0;
}

// clipf[seg] = the smallest whole-batch index of an overflowing frame of seg.
// The lanes of a wave that overflow are grouped by segment with a ballot
// loop (wave-uniform; a segment's frames are contiguous, so a wave sees few):
// the lowest lane of a group holds its minimum and issues the one atomicMin.
__global__ __launch_bounds__(TR_T) void ord_clip_first_k(
    OrdClip c, const uint8_t* __restrict__ rank, int64_t ncap,
    int32_t passes) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int64_t nfr = *c.nall;
  if (nfr > ncap) nfr = ncap;
  int32_t seg = -1;
  bool ov = false;
  if (i < nfr) {
    seg = c.f_seg[i];
    ov = seg >= 0 && seg < c.S && (c.bad == nullptr || *c.bad == 0) &&
         clip_overflow(c.cls[i], c.sub[i], rank, ncap, passes);
  }
  uint64_t m = __ballot(ov);
  while (m != 0) {
    const int l = __ffsll((unsigned long long)m) - 1;
    const int32_t sl = __shfl(seg, l, 64);
    const uint64_t same = __ballot(ov && seg == sl);
    if (lane == l)
      atomicMin((unsigned long long*)&c.clipf[sl], (unsigned long long)i);
    m &= ~same;
  }
}

// Frame i at or after its segment's clipf leaves the batch.  A frame of the
// serve's class also gets the rank byte ORD_RANK (rank, when the ordered
// serve follows): the last pass answers it, and the serve's DEFER instance
// tells it from a frame of a batch refused as a whole (tree.hip: a deferred
// SEQUENTIAL create keeps its number out of use, a gap in the parent's
// cversion, where the whole refusal hands the numbers back).
__global__ __launch_bounds__(TR_T) void ord_clip_mark_k(
    OrdClip c, int64_t ncap, uint8_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  int64_t nfr = *c.nall;
  if (nfr > ncap) nfr = ncap;
  bool df = false;
  if (i < nfr) {
    df = clip_deferred(c.clipf, c.S, c.f_seg[i], i);
    if (df) {
      c.f_seg[i] = -1;
      const int32_t k = c.cls[i], sb = c.sub[i];
      if (k >= 0 && k < MIX_CLASSES && sb >= 0 && sb < ncap)
        (k == 0 ? c.seg_c[0] : k == 1 ? c.seg_c[1] : c.seg_c[2])[sb] = -1;
      if (k == MIX_A && sb >= 0 && sb < ncap && rank != nullptr)
        rank[sb] = (uint8_t)ORD_RANK;
    }
  }
  const uint64_t m = __ballot(df);
  if (m != 0 && (threadIdx.x & 63) == 0)
    atomicAdd((unsigned long long*)c.deferred,
              (unsigned long long)__popcll((unsigned long long)m));
}

__global__ __launch_bounds__(TR_T) void ord_clip_ranges_k(
    const int64_t* __restrict__ clipf, const int64_t* __restrict__ rep_off,
    const int64_t* __restrict__ rec_off, const int64_t* __restrict__ off,
    const int64_t* __restrict__ starts, const int64_t* __restrict__ nall,
    int64_t ncap, int64_t S, int64_t* __restrict__ rep_end,
    int64_t* __restrict__ used) {
  const int64_t s = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (s >= S) return;
  int64_t nfr = *nall;
  if (nfr > ncap) nfr = ncap;
  const ClipRange r = clip_range(clipf, rep_off, rec_off, off, starts, nfr, s);
  rep_end[s] = r.rep_end;
  used[s] = r.used;
}

static_assert(CLIP_RANK == ORD_RANK, "zk_order_clip.h: the rank bits");

// mark_rank: the rank table is the ordered serve's own (not a caller's).
int clip_launch(const ZkOrdClip& clip, uint8_t* rank, int64_t ncap,
                int32_t passes, bool mark_rank, hipStream_t st) {
  const OrdClip c{clip};
  if (ncap < 1 || ncap > 0x7fffffff || c.S < 1 || c.S > 0x7fffffff ||
      passes < 1)
    return -1;
  const unsigned nb = (unsigned)((ncap + TR_T - 1) / TR_T);
  ord_clip_init_k<<<(unsigned)((c.S + TR_T - 1) / TR_T), TR_T, 0, st>>>(c,
                                                                        ncap);
  ZK_LAUNCH_CHECK();
  ord_clip_first_k<<<nb, TR_T, 0, st>>>(c, rank, ncap, passes);
  ZK_LAUNCH_CHECK();
  ord_clip_mark_k<<<nb, TR_T, 0, st>>>(c, ncap, mark_rank ? rank : nullptr);
  ZK_LAUNCH_CHECK();
  return 0;
}

int bscan_launch(int64_t* bsum, int64_t nb, hipStream_t st) {
  ord_bscan_k<<<1, ORD_SCAN_T, 0, st>>>(bsum, nb);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace zk

extern "C" {

// Ordering workspace layout for up to ncap requests: the zeroed prefix
// (counters, key, cw, fill, lastw), then base, bsum, eidx, members, rank.
static int64_t order_hcap(int64_t ncap) {
  int64_t h = 1024;
  while (h < 2 * ncap) h <<= 1;
  return h;
}

static int64_t order_layout(int64_t ncap, uint8_t* ws, zk::OrderWs* w,
                            uint8_t** rank, int64_t* zeroed) {
  const int64_t h = order_hcap(ncap);
  int64_t o = 32;
  if (w != nullptr) {
    w->ctr = (int64_t*)ws;
    w->key = (int64_t*)(ws + o);
  }
  o += h * 8;
  if (w != nullptr) w->cnt = (int64_t*)(ws + o);
  o += h * 8;
  if (w != nullptr) w->fill = (int32_t*)(ws + o);
  o += h * 4;
  if (w != nullptr) w->lastw = (int32_t*)(ws + o);
  o += h * 4;
  if (zeroed != nullptr) *zeroed = o;
  if (w != nullptr) w->base = (int32_t*)(ws + o);
  o += h * 4;
  if (w != nullptr) w->bsum = (int64_t*)(ws + o);
  o += (h / zk::TR_T) * 8;
  if (w != nullptr) w->eidx = (int64_t*)(ws + o);
  o += 2 * ncap * 8;
  if (w != nullptr) w->members = (int32_t*)(ws + o);
  o += 2 * ncap * 4;
  if (w != nullptr) w->rnk = (int32_t*)(ws + o);
  o += ncap * 4;
  if (rank != nullptr) *rank = ws + o;
  o += ncap;
  if (w != nullptr) w->mask = h - 1;
  return o;
}

// A deferral's tables: every one of them given, at least one segment.
static bool clip_ok(const ZkOrdClip* c) {
  return c != nullptr && c->cls != nullptr && c->sub != nullptr &&
         c->nall != nullptr && c->f_seg != nullptr &&
         c->seg_c[0] != nullptr && c->seg_c[1] != nullptr &&
         c->seg_c[2] != nullptr && c->clipf != nullptr &&
         c->deferred != nullptr && c->S >= 1;
}

// Bytes of the ordering workspace for up to ncap requests.
int64_t zk_tree_order_workspace(int64_t ncap) {
  return order_layout(ncap, nullptr, nullptr, nullptr, nullptr);
}

// zk_tree_serve with the batch applied in path order: rank every request
// (ord_* above), then `passes` serve launches of increasing rank (each
// followed by the parent fix-up; the free nodes are published and the
// batch's zxids consumed by the last).  A request of rank >= passes is
// answered SYSTEMERROR and shows in the max rank (zk_tree_order_stats_offset;
// the caller can read it and use more passes).  The launches do not depend
// on the ranks: no host read.
// (segs: a session batch's table; null: one session, one watcher slot.  clip,
// with segs: deferral in place of the rank refusal, see below)
static int ordered_serve(const ZkTree* t, const uint8_t* rx, const ZkReqOut* q,
                         const int64_t* n_dev, int64_t ncap,
                         const ZkServeOut* out, int64_t session,
                         int64_t now_ms, uint8_t* ws, int64_t ws_bytes,
                         int32_t passes, int64_t snap_base, int64_t snap_cap,
                         int32_t wslot, int64_t* fired,
                         const ZkSegs* segs, const ZkOrdClip* clip,
                         hipStream_t st) {
  if (ncap <= 0) return 0;
  if (ncap > zk::ORD_FM) return -1;          // packed group counts
  if (passes < 1 || passes > zk::ORD_RANK) return -1;
  if (snap_base < 0 || snap_cap < 0 || (snap_base & 15)) return -1;
  if (ws_bytes < zk_tree_order_workspace(ncap)) return -1;
  if (((uintptr_t)ws & 15) != 0) return -1;
  zk::OrderWs w;
  uint8_t* rank = nullptr;
  int64_t zeroed = 0;
  order_layout(ncap, ws, &w, &rank, &zeroed);
  const int64_t h = w.mask + 1;
  if (hipMemsetAsync(ws, 0, (size_t)zeroed, st) != hipSuccess) return -4;
  const unsigned nb = (unsigned)((ncap + zk::TR_T - 1) / zk::TR_T);
  zk::ord_insert_k<<<nb, zk::TR_T, 0, st>>>(rx, *q, n_dev, ncap, w);
  ZK_LAUNCH_CHECK();
  zk::ord_base_k<<<(unsigned)(h / zk::TR_T), zk::TR_T, 0, st>>>(w);
  ZK_LAUNCH_CHECK();
  int rc = zk::bscan_launch(w.bsum, h / zk::TR_T, st);
  if (rc) return rc;
  zk::ord_fill_k<<<nb, zk::TR_T, 0, st>>>(ncap, w);
  ZK_LAUNCH_CHECK();
  // ranks of chains up to `passes` long are exact after passes + 1 rounds
  // (a longer chain ends at rank >= passes: refused either way)
  for (int32_t r = 0; r <= passes; ++r) {
    zk::ord_relax_k<<<nb, zk::TR_T, 0, st>>>(ncap, w);
    ZK_LAUNCH_CHECK();
  }
  zk::ord_rank_k<<<nb, zk::TR_T, 0, st>>>(ncap, w, rank);
  ZK_LAUNCH_CHECK();
  if (clip != nullptr) {
    // deferral: the frames the passes cannot reach leave the batch
    rc = zk::clip_launch(*clip, rank, ncap, passes, true, st);
    if (rc) return rc;
  }
  zk::ServeLaunch s;
  s.tree = t, s.rx = rx, s.q = q, s.n_dev = n_dev, s.ncap = ncap;
  s.out = out, s.session = session, s.now_ms = now_ms, s.rank = rank;
  s.snap_base = snap_base, s.snap_cap = snap_cap, s.snap_top = &w.ctr[2];
  s.wslot = wslot, s.fired = fired;
  s.segs = segs, s.defer = clip != nullptr;
  for (s.pass = 0; s.pass < passes; ++s.pass) {
    const int32_t last = s.pass == passes - 1;
    s.last_pass = last;
    rc = zk::serve_launch(s, st);
    if (rc) return rc;
    // nodes freed by a pass are recycled from the next batch on: a reply of
    // this batch may still name them
    rc = zk::finish_launch(t, last ? n_dev : nullptr, 0, last, st);
    if (rc) return rc;
  }
  return 0;
}

int zk_tree_serve_ordered(const ZkTree* t, const uint8_t* rx, const ZkReqOut* q,
                          const int64_t* n_dev, int64_t ncap,
                          const ZkServeOut* out, int64_t session,
                          int64_t now_ms, uint8_t* ws, int64_t ws_bytes,
                          int32_t passes, int64_t snap_base, int64_t snap_cap,
                          int32_t wslot, int64_t* fired, hipStream_t st) {
  return ordered_serve(t, rx, q, n_dev, ncap, out, session, now_ms, ws,
                       ws_bytes, passes, snap_base, snap_cap, wslot, fired,
                       nullptr, nullptr, st);
}

// zk_tree_serve_ordered for a session batch (segs: ZkSegs): requests on one
// path are applied in stream order whichever segments they come from.
// clip (or null): over the serve's class of a session batch of any op mix,
// deferral in place of the rank refusal (ord_clip_* above; the rules:
// zk_order_clip.h).  (rx .. segs) are then the class's compacted frames —
// segs->f_seg is clip->seg_c[0] — and clip the WHOLE batch's tables.  Three
// launches between the ranking and the first pass; no host read.
int zk_tree_serve_ordered_sessions(
    const ZkTree* t, const uint8_t* rx, const ZkReqOut* q,
    const int64_t* n_dev, int64_t ncap, const ZkServeOut* out, int64_t now_ms,
    uint8_t* ws, int64_t ws_bytes, int32_t passes, int64_t snap_base,
    int64_t snap_cap, int64_t* fired, const ZkSegs* segs,
    const ZkOrdClip* clip, hipStream_t st) {
  if (segs == nullptr || segs->f_seg == nullptr ||
      (clip != nullptr &&
       (!clip_ok(clip) || clip->seg_c[0] != segs->f_seg ||
        clip->S != segs->S || clip->bad != segs->bad)))
    return (int)hipErrorInvalidValue;
  return ordered_serve(t, rx, q, n_dev, ncap, out, 0, now_ms, ws, ws_bytes,
                       passes, snap_base, snap_cap, -1, fired, segs, clip, st);
}

// The deferral stage alone (the three launches), over a rank table of the
// caller's: rank[ncap] and the tables (bad null).
int zk_order_clip(const uint8_t* rank, int32_t passes, const ZkOrdClip* clip,
                  int64_t ncap, hipStream_t st) {
  if (rank == nullptr || !clip_ok(clip) || clip->bad != nullptr || ncap < 1)
    return (int)hipErrorInvalidValue;
  // (the caller's rank table is only read)
  return zk::clip_launch(*clip, const_cast<uint8_t*>(rank), ncap, passes,
                         false, st);
}

// After the merge and zk_sess_ranges: per segment where its replies end and
// how many of its request bytes were consumed (zk_order_clip.h clip_range).
// clipf[S], rep_off[S + 1], the merged rec_off[ncap], the whole batch's frame
// table off[ncap] and count nall, starts[S + 1] -> rep_end[S], used[S].
int zk_order_clip_ranges(const int64_t* clipf, const int64_t* rep_off,
                         const int64_t* rec_off, const int64_t* off,
                         const int64_t* starts, const int64_t* nall,
                         int64_t ncap, int64_t S, int64_t* rep_end,
                         int64_t* used, hipStream_t st) {
  if (S < 1 || S > 0x7fffffff || ncap < 0) return (int)hipErrorInvalidValue;
  zk::ord_clip_ranges_k<<<(unsigned)((S + zk::TR_T - 1) / zk::TR_T), zk::TR_T,
                          0, st>>>(clipf, rep_off, rec_off, off, starts, nall,
                                   ncap, S, rep_end, used);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Byte offset in the ordering workspace of {max rank, scratch bytes used}
// of the last ordered serve (int64 each; read them after the stream).
int64_t zk_tree_order_stats_offset(int64_t ncap) {
  (void)ncap;
  return 8;
}

}  // extern "C"
