// The GPU tree's SEQUENTIAL numbering pass (the tree: zk_tree.h; the serve
// reads the numbers through ZkTree.seqno, tree.hip seq_num / seq_par).
#include "zk_tree.h"

namespace zk {

// ---- SEQUENTIAL numbers in stream order (seq_*) ----------------------------
// A ZooKeeper leader names a SEQUENTIAL create once, from the parent's
// cversion when it prepares the txn, in zxid order; followers apply the
// name.  The serve applies a batch's creates concurrently, so a number
// taken from an atomic at create time follows wave scheduling: one
// session's pipelined creates came out in any order, and the members of a
// replicated tree, each re-executing the same batch, named them
// differently.  Here every SEQUENTIAL create of a batch is numbered
//     base(parent) + its rank among the batch's SEQUENTIAL creates under
//     that parent, in stream order,
// base being the parent's cversion before the batch, which then moves once
// by the group's size (a create that fails leaves a gap).  The numbers are
// a function of the batch and the tree before it: the same on every
// member and every run (reference: test/basic.test.js:550-611 names;
// test/multi-node.test.js:107-165 one tree behind every member).
//
// Five launches, no host read, O(n) work apart from a 1024-element LDS
// sort per chunk; a group is named by its slot e in a scratch hash of the
// parent paths (no dense ids: nothing waits for another workgroup):
//  1. seq_group_k, one 1024-request chunk per workgroup: parse, the parent
//     path's slot, the chunk's (slot, lane) pairs sorted in LDS (bitonic):
//     each request's rank in its chunk and group, each (group, chunk)
//     count, the group's chunk bit; a new group goes on the group list;
//  2. seq_alloc_k: per group, one count slot per chunk it appears in, and
//     the bitmap's per-word popcount prefix;
//  3. seq_index_k: per request, its chunk's index among its group's chunks
//     (chunk order = stream order); chunk leaders store their counts there;
//  4. seq_scan_k, a wave per group: exclusive scan of its chunk counts;
//     the parent looked up and bumped once; scratch left zero;
//  5. seq_out_k: number = base + chunk prefix + rank in the chunk.
// A group is keyed by the 64-bit hash of the parent path (a collision merges
// two parents' numbering: 2^-64 a pair).  A parent the pass does not find
// (created in the same batch) leaves its creates to the serve's atomic.
// (A first version gave groups dense ids, published by the claiming
// workgroup while the others spun on them: 134 us of the storm's 1M-create
// step in seq_group_k alone.)
constexpr int SQ_C = 1024;                 // requests per chunk (workgroup)
constexpr int64_t SQ_MAX = 1 << 24;        // requests a batch

struct SeqWs {
  int64_t* ctr;       // [8] groups, count slots used
  int64_t* key;       // [h] parent path hash | 1 (0 empty)
  uint64_t* mask;     // [h * mw] chunk bitmap per group slot
  uint16_t* pp;       // [h * mw] popcount of the bitmap words before
  int64_t* goff;      // [h] group -> its first count slot
  int32_t* gbase;     // [h] group -> parent cversion before the batch (-1)
  int32_t* gpar;      // [h] group -> its parent node
  int32_t* rep;       // [h] group -> one of its requests
  int32_t* glist;     // [ncap] the batch's group slots
  int32_t* cnts;      // [ncap] chunk counts, then their group prefixes
  int32_t* gid;       // [ncap] request -> group slot (-1)
  int32_t* rin;       // [ncap] request -> rank within its chunk and group
  int32_t* lcnt;      // [ncap] chunk leader -> its group's count there
  int32_t* kk;        // [ncap] request -> its chunk among its group's chunks
  int64_t hmask;
  int32_t mw;         // bitmap words per group (<= SQ_MW)
  int64_t* dbg;       // optional: 4 phase clocks per chunk (zk_tree_seq_debug)
};

// The parent path of a SEQUENTIAL create frame ([p, p + cut)); cut 0 for
// anything else (a root child has no parent node either).  Only what the
// numbering needs is read — the op, the path and the flags, the frame's
// last word — in three dependent loads, not the full parse's walk of the
// data and ACL (whose many dependent loads, a million frames in flight,
// re-fetched the stream's lines ~3x: 300 MB for an 83 MB batch).  A frame
// the serve's full parse then refuses is un-numbered there (tree_serve_k).
ZK_DEV int32_t seq_parent(const uint8_t* rx, int64_t off, int32_t len,
                          const uint8_t** p) {
  if (len < 28) return 0;            // xid op path(4) data(4) acl(4) flags
  const uint8_t* b = rx + off;
  uint32_t h[3];
  __builtin_memcpy(h, b, 12);
  const int32_t pl = (int32_t)bswap32(h[2]);
  // (64-bit: a path length word near 2^31 overflowed `12 + pl + 12` as int
  // and passed, and the '/' search then read 2 GiB past the frame)
  if ((int32_t)bswap32(h[1]) != OP_CREATE || pl < 2 || (int64_t)pl + 24 > len)
    return 0;
  if (!(ld_be32(b + len - 4) & CF_SEQUENTIAL)) return 0;
  *p = b + 12;
  int32_t cut = pl - 1;
  while (cut > 0 && (*p)[cut] != '/') --cut;
  return cut;
}

// The group key (path_hash of the parent path | 1; 0: not a SEQUENTIAL
// create) of the create frame [b, b + len): the frame's first 64 bytes and
// its last word are loaded at once — one round trip after the frame table,
// not seq_parent's chain of a header load, the flags load, a byte load per
// step of the '/' search and the hash's own loads (the probe's clocks: 32
// us a chunk for those, tools/microbench/seq_probe.py) — and the op, the
// flags, the last '/' and the hash come from registers.  A path past the
// 64 bytes (pl > 52) or a frame under them takes seq_parent.
ZK_DEV uint64_t seq_key(const uint8_t* rx, int64_t off, int32_t len) {
  if (len < 64) {
    const uint8_t* p = nullptr;
    const int32_t cut = seq_parent(rx, off, len, &p);
    return cut > 0 ? path_hash(p, cut) | 1ull : 0;
  }
  const uint8_t* b = rx + off;
  uint32_t W[16], fl;
  __builtin_memcpy(W, b, 64);
  __builtin_memcpy(&fl, b + len - 4, 4);
  // (every load issued before the first test: the compiler otherwise sinks
  // the path words and the flags below the op test, one wait each)
  asm volatile("" ::"v"(W[0]), "v"(W[1]), "v"(W[2]), "v"(W[3]), "v"(W[4]),
               "v"(W[5]), "v"(W[6]), "v"(W[7]), "v"(W[8]), "v"(W[9]),
               "v"(W[10]), "v"(W[11]), "v"(W[12]), "v"(W[13]), "v"(W[14]),
               "v"(W[15]), "v"(fl));
  const int32_t pl = (int32_t)bswap32(W[2]);
  if ((int32_t)bswap32(W[1]) != OP_CREATE || pl < 2 || (int64_t)pl + 24 > len ||
      !(bswap32(fl) & CF_SEQUENTIAL))
    return 0;
  if (pl > 52) {
    const uint8_t* p = nullptr;
    const int32_t cut = seq_parent(rx, off, len, &p);
    return cut > 0 ? path_hash(p, cut) | 1ull : 0;
  }
  // '/' bytes of path positions 1 .. pl - 1 (path byte q: word 3 + q / 4)
  uint64_t slash = 0;
#pragma unroll
  for (int k = 3; k < 16; ++k) {
    const uint32_t x = W[k] ^ 0x2F2F2F2Fu;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    const uint64_t nib = ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) |
                         ((z >> 28) & 8u);
    slash |= nib << (4 * (k - 3));
  }
  slash &= ((1ull << pl) - 1) & ~1ull;
  if (!slash) return 0;
  const int32_t cut = 63 - __builtin_clzll(slash);
  // path_hash(path, cut) from the words: 8-byte pieces, the last masked
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)cut;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    if (8 * j < cut) {
      uint64_t x = (uint64_t)W[3 + 2 * j] | (uint64_t)W[4 + 2 * j] << 32;
      const int32_t left = cut - 8 * j;
      if (left < 8) x &= (1ull << (8 * left)) - 1;
      h = (h ^ x) * 0xFF51AFD7ED558CCDull;
      h ^= h >> 32;
    }
  }
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return h | 1ull;
}

// Within the chunk, each request's rank among the chunk's requests of its
// group (in lane = stream order) and each group's count, without a sort:
// the group slots get chunk-local dense ids through an LDS hash, a wave
// finds each lane's peers (same id) with one ballot per distinct id, and
// per-wave counts cnt[wave][id] in LDS give the count of the waves before.
// Four barriers; a bitonic sort of the chunk's 1024 (slot, lane) pairs
// took 75 barrier stages: 44 us a launch with nothing to sort, 145 us for
// the storm's 1M creates.
constexpr int SQ_W = SQ_C / 64;              // waves a chunk
constexpr int SQ_LH = 2 * SQ_C;              // LDS hash slots
__global__ __launch_bounds__(SQ_C) void seq_group_k(
    const uint8_t* __restrict__ rx, const int64_t* __restrict__ foff,
    const int32_t* __restrict__ flen, const int64_t* __restrict__ n_dev,
    int64_t ncap, SeqWs w) {
  __shared__ int32_t lkey[SQ_LH];            // group slot e (-1 empty)
  __shared__ int32_t lid[SQ_LH];             // its chunk-local dense id
  __shared__ uint16_t cnt[SQ_W][SQ_C];       // [wave][dense id] counts
  __shared__ int32_t ndense;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t c = blockIdx.x;
  const int64_t i = c * SQ_C + tid;
  int64_t* const dbg = w.dbg ? w.dbg + 5 * c : nullptr;
  if (dbg && tid == 0) dbg[0] = wall_clock64();
  // (the frame table and the count loaded together)
  const int64_t fo = i < ncap ? foff[i] : 0;
  const int32_t fn = i < ncap ? flen[i] : 0;
  const bool in = i < ncap && i < *n_dev;
  int64_t e = -1;
  bool first = false;
  const int64_t key = in ? (int64_t)seq_key(rx, fo, fn) : 0;
  if (dbg) {
    __syncthreads();
    if (tid == 0) dbg[4] = wall_clock64();
  }
  {
    if (key != 0) {
      int64_t s = key & w.hmask;
      for (int64_t probe = 0; probe <= w.hmask; ++probe) {
        // a plain load first (a stale 0 only means the CAS answers)
        int64_t k = w.key[s];
        if (k == 0)
          k = (int64_t)atomicCAS((unsigned long long*)&w.key[s], 0ull,
                                 (unsigned long long)key);
        if (k == 0) { first = true; e = s; break; }
        if (k == key) { e = s; break; }
        s = (s + 1) & w.hmask;
      }
    }
  }
  if (i < ncap) {
    w.lcnt[i] = 0;
    w.gid[i] = (int32_t)e;
  }
  // the group list: one ticket per new group, one atomic per workgroup
  const int64_t k = block_ticket<SQ_C>(&w.ctr[0], first);
  if (first) {
    w.glist[k] = (int32_t)e;
    w.rep[e] = (int32_t)i;
  }
  if (dbg && tid == 0) dbg[1] = wall_clock64();   // (after the ticket's barriers)
  if (!__syncthreads_or(e >= 0)) return;     // (block-uniform)
  // 1. chunk-local dense ids
  for (int x = tid; x < SQ_LH; x += SQ_C) lkey[x] = -1;
  for (int x = tid; x < SQ_C * SQ_W / 2; x += SQ_C)
    reinterpret_cast<uint32_t*>(&cnt[0][0])[x] = 0;   // (uint16 pairs)
  if (tid == 0) ndense = 0;
  __syncthreads();
  int ls = -1;
  if (e >= 0) {
    const int32_t ek = (int32_t)e;
    ls = (int)(((uint32_t)ek * 2654435761u) >> 21) & (SQ_LH - 1);
    for (;;) {
      const int32_t o = atomicCAS(&lkey[ls], -1, ek);
      if (o == -1) {
        lid[ls] = atomicAdd(&ndense, 1);
        break;
      }
      if (o == ek) break;
      ls = (ls + 1) & (SQ_LH - 1);
    }
  }
  __syncthreads();
  if (dbg && tid == 0) dbg[2] = wall_clock64();
  const int d = e >= 0 ? lid[ls] : -1;
  // 2. peers in the wave: one ballot per distinct id
  uint64_t peers = 0;
  uint64_t todo = __ballot(d >= 0);
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    const int dk = __shfl(d, src, 64);
    const uint64_t m = __ballot(d == dk);
    if (d == dk) peers = m;
    todo &= ~m;
  }
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int rw = __popcll(peers & below);
  if (d >= 0 && rw == 0) cnt[wv][d] = (uint16_t)__popcll(peers);
  __syncthreads();
  // 3. the waves before, the chunk's count (its first request leads)
  if (d >= 0) {
    int pre = 0, tot = 0;
#pragma unroll
    for (int x = 0; x < SQ_W; ++x) {
      const int v = cnt[x][d];
      pre += x < wv ? v : 0;
      tot += v;
    }
    w.rin[i] = pre + rw;
    if (pre + rw == 0) {
      w.lcnt[i] = tot;
      atomicOr((unsigned long long*)&w.mask[e * w.mw + (c >> 6)],
               1ull << (c & 63));
    }
  }
  if (dbg) {
    __syncthreads();
    if (tid == 0) dbg[3] = wall_clock64();
  }
}

__global__ __launch_bounds__(TR_T) void seq_alloc_k(SeqWs w) {
  const int64_t ng = w.ctr[0];
  const int64_t stride = (int64_t)gridDim.x * TR_T;
  // (g0 is wave-uniform: wave_bytes needs the whole wave)
  for (int64_t g0 = (int64_t)blockIdx.x * TR_T + (threadIdx.x & ~63);
       g0 < ng; g0 += stride) {
    const int64_t g = g0 + (threadIdx.x & 63);
    const int64_t e = g < ng ? w.glist[g] : -1;
    int64_t n = 0;
    if (e >= 0) {
      const uint64_t* m = w.mask + e * w.mw;
      uint16_t* pp = w.pp + e * w.mw;
      for (int k = 0; k < w.mw; ++k) {
        pp[k] = (uint16_t)n;
        n += __popcll(m[k]);
      }
    }
    const int64_t o = wave_bytes(&w.ctr[1], n);
    if (e >= 0) w.goff[e] = o;
  }
}

__global__ __launch_bounds__(TR_T) void seq_index_k(int64_t ncap, SeqWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  const int64_t e = w.gid[i];
  if (e < 0) return;
  const int64_t c = i / SQ_C;
  const int64_t wd = e * w.mw + (c >> 6);
  const int32_t x = (int32_t)w.pp[wd] +
                    __popcll(w.mask[wd] & ((1ull << (c & 63)) - 1));
  w.kk[i] = x;
  const int32_t lc = w.lcnt[i];
  if (lc > 0) w.cnts[w.goff[e] + x] = lc;
}

__global__ __launch_bounds__(TR_T) void seq_scan_k(
    ZkTree t, const uint8_t* __restrict__ rx, const int64_t* __restrict__ foff,
    const int32_t* __restrict__ flen, SeqWs w) {
  const int lane = threadIdx.x & 63;
  const int64_t ng = w.ctr[0];
  const int64_t nwv = ((int64_t)gridDim.x * TR_T) >> 6;
  for (int64_t g = ((int64_t)blockIdx.x * TR_T + threadIdx.x) >> 6; g < ng;
       g += nwv) {
    const int64_t e = w.glist[g];
    uint64_t* m = w.mask + e * w.mw;
    int64_t n = 0;
    for (int k = lane; k < w.mw; k += 64) n += __popcll(m[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    const int64_t o = w.goff[e];
    int64_t run = 0;
    for (int64_t b = 0; b < n; b += 64) {
      const int64_t j = b + lane;
      const int64_t x = j < n ? w.cnts[o + j] : 0;
      const int64_t inc = wave_incl_scan(x);
      if (j < n) w.cnts[o + j] = (int32_t)(run + inc - x);
      run += __shfl(inc, 63, 64);
    }
    // the parent, found and bumped once for the whole group
    if (lane == 0) {
      int32_t base = -1;
      const int32_t r = w.rep[e];
      const uint8_t* p = nullptr;
      const int32_t cut = seq_parent(rx, foff[r], flen[r], &p);
      const int64_t par = cut > 0 ? tree_find(t, p, cut) : -1;
      // cversion and numChildren move by the group's size in one atomic
      // (the serve takes a failed create's child back)
      if (par >= 0 && t.eph[par] == 0)
        base = cn_cver(cn_add(t, par, (int32_t)run, (int32_t)run));
      w.gbase[e] = base;
      w.gpar[e] = (int32_t)par;
      w.key[e] = 0;
    }
    for (int k = lane; k < w.mw; k += 64) m[k] = 0;
  }
}

__global__ __launch_bounds__(TR_T) void seq_out_k(int64_t ncap, SeqWs w,
                                                  int64_t* __restrict__ seqno) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  const int64_t e = w.gid[i];
  int64_t s = -1;
  if (e >= 0) {
    const int32_t b = w.gbase[e];
    const int32_t x = b >= 0 ? b + w.cnts[w.goff[e] + w.kk[i]] + w.rin[i] : -1;
    if (x >= 0) s = ((int64_t)w.gpar[e] << 32) | (uint32_t)x;
  }
  seqno[i] = s;
}

}  // namespace zk

extern "C" {

// Workspace of zk_tree_seq_order: the prefix that must start zeroed (and is
// left zeroed: hash keys, published ids, chunk bitmaps), then the counters
// (reset every call) and the per-group / per-request arrays.
static int64_t seq_layout(int64_t ncap, uint8_t* ws, zk::SeqWs* w,
                          int64_t* zeroed) {
  int64_t h = 1024;
  while (h < 2 * ncap) h <<= 1;
  const int64_t nch = (ncap + zk::SQ_C - 1) / zk::SQ_C;
  const int32_t mw = (int32_t)((nch + 63) / 64 > 0 ? (nch + 63) / 64 : 1);
  auto at = [&](int64_t o) { return ws != nullptr ? ws + o : nullptr; };
  auto a16 = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  int64_t o = 0;
  if (w != nullptr) {
    w->hmask = h - 1;
    w->mw = mw;
    w->key = (int64_t*)at(o);
  }
  o += h * 8;
  if (w != nullptr) w->mask = (uint64_t*)at(o);
  o += h * mw * 8;
  if (zeroed != nullptr) *zeroed = o;
  if (w != nullptr) w->ctr = (int64_t*)at(o);
  o += 64;
  if (w != nullptr) w->pp = (uint16_t*)at(o);
  o += a16(h * mw * 2);
  if (w != nullptr) w->goff = (int64_t*)at(o);
  o += h * 8;
  if (w != nullptr) w->gbase = (int32_t*)at(o);
  o += h * 4;
  if (w != nullptr) w->rep = (int32_t*)at(o);
  o += h * 4;
  if (w != nullptr) w->gpar = (int32_t*)at(o);
  o += h * 4;
  int32_t** arr[] = {w ? &w->glist : nullptr, w ? &w->cnts : nullptr,
                     w ? &w->gid : nullptr,   w ? &w->rin : nullptr,
                     w ? &w->lcnt : nullptr,  w ? &w->kk : nullptr};
  for (int32_t** p : arr) {
    if (p != nullptr) *p = (int32_t*)at(o);
    o += a16(ncap * 4);
  }
  return o;
}

// Phase clocks of seq_group_k (tools/microbench/seq_probe.py): buf holds
// 5 int64 per 1024-request chunk — start, the key table probe and group
// ticket done, chunk-local ids done, end, and (an extra barrier) the parse
// done (wall_clock64 ticks, 100 MHz); nullptr turns them off.
static int64_t* g_seq_dbg = nullptr;
void zk_tree_seq_debug(int64_t* buf) { g_seq_dbg = buf; }

int64_t zk_tree_seq_workspace(int64_t ncap) {
  return ncap > 0 ? seq_layout(ncap, nullptr, nullptr, nullptr) : 0;
}

int64_t zk_tree_seq_zeroed(int64_t ncap) {
  int64_t z = 0;
  if (ncap > 0) seq_layout(ncap, nullptr, nullptr, &z);
  return z;
}

// SEQUENTIAL numbers of the batch's create frames (foff / flen, *n_dev of
// them) in stream order -> seqno[ncap] (parent node << 32 | number; -1:
// none); see seq_* above.  Run
// it before the serve of the same frames, with t->seqno = seqno there.
int zk_tree_seq_order(const ZkTree* t, const uint8_t* rx, const int64_t* foff,
                      const int32_t* flen, const int64_t* n_dev, int64_t ncap,
                      uint8_t* ws, int64_t ws_bytes, int64_t* seqno,
                      hipStream_t st) {
  if (ncap <= 0) return 0;
  if (ncap > zk::SQ_MAX) return -1;
  if (ws_bytes < zk_tree_seq_workspace(ncap) || ((uintptr_t)ws & 15))
    return -1;
  zk::SeqWs w;
  int64_t zeroed = 0;
  seq_layout(ncap, ws, &w, &zeroed);
  w.dbg = g_seq_dbg;
  if (hipMemsetAsync(w.ctr, 0, 64, st) != hipSuccess) return -4;
  const unsigned nchunk = (unsigned)((ncap + zk::SQ_C - 1) / zk::SQ_C);
  const unsigned nb = (unsigned)((ncap + zk::TR_T - 1) / zk::TR_T);
  const unsigned ng = nb < 1024 ? nb : 1024;   // grid-stride over groups
  zk::seq_group_k<<<nchunk, zk::SQ_C, 0, st>>>(rx, foff, flen, n_dev, ncap, w);
  ZK_LAUNCH_CHECK();
  zk::seq_alloc_k<<<ng, zk::TR_T, 0, st>>>(w);
  ZK_LAUNCH_CHECK();
  zk::seq_index_k<<<nb, zk::TR_T, 0, st>>>(ncap, w);
  ZK_LAUNCH_CHECK();
  zk::seq_scan_k<<<ng, zk::TR_T, 0, st>>>(*t, rx, foff, flen, w);
  ZK_LAUNCH_CHECK();
  zk::seq_out_k<<<nb, zk::TR_T, 0, st>>>(ncap, w, seqno);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
