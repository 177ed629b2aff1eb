// Mixed batches on the GPU server (GpuServer.serve_mixed): a split in front
// of the three serve engines and a merge behind them.
//
// The engines — the fused serve (tree.hip), the GET_ACL path (tree_acl.hip)
// and the list path (tree_list.hip) — each take a frame table with a device
// count and return a reply stream with rec_off[] and a device total.  So a
// batch of any op mix is served by
//   split   the batch's K1 frame table -> the class of every frame
//           (zk_mix.h mix_class), its index inside the class and three
//           compacted frame tables with device counts, stable (request order
//           kept inside a class): route.hip's shape with three "owners" —
//           mix_class_k (class + per-block histogram), the device-wide scan
//           in class-major order, mix_scatter_k (ballot ranks + an LDS prefix
//           over waves).  No host read, no shared counter.
//   (the three engines on their sub-tables, each into a stream of its own)
//   merge   request i of class c, index j: its reply is bytes
//           [rec_off_c[j], rec_off_c[j + 1]) of stream c (the class's last
//           reply ends at total_c).  mix_size_k (sizes and source offsets;
//           replies past MIX_WAVE queue up for the whole grid), the
//           device-wide scan (the merged rec_off and total), mix_total_k
//           (err, capacity, terminator: list_total_k's conventions), then the
//           copies.
//
// The copy (the hot path).  Replies run from 20 bytes to megabytes, and the
// source and destination alignments are arbitrary and differ.  Every tier
// writes the destination's aligned interior with 16-byte stores; the source
// is read as aligned 16-byte words (one, or two where it sits across) and
// funnel-shifted into place (alignbyte, as K13's hole copy does), all loads
// of a trip issued before its first store; the ragged head and tail (at most
// 15 bytes each) go byte by byte, so a reply's lanes write exactly its bytes.
//   tier 1  size <= MIX_SMALL = 256 B: MIX_G = 8 lanes a reply, two 16-byte
//           units a lane a trip — one trip covers the reply (a GET_DATA reply
//           of the bench tree is 192 B, a GET_ACL reply ~115 B, a header 20),
//           and a wave's 8 neighbouring replies store one contiguous span, as
//           acl_write_k's do.
//   tier 2  MIX_SMALL < size <= MIX_WAVE = 64 KiB: a wave a reply, four units
//           a lane a trip (4 KiB a trip, 16 trips at the bound), as
//           list_copy_k: after tier 1 a wave takes those of its 8 requests
//           one at a time with all its lanes.  Both tiers are mix_copy_k.
//   tier 3  size > MIX_WAVE (a list of a large directory): one wave's serial
//           trips would be the batch's critical path, so mix_size_k queues
//           these replies and the MIX_HUGE_WG workgroups of mix_copy_huge_k
//           (4096 waves) share the queue out: a group of waves per reply, the
//           reply's 4 KiB chunks round robin inside it.
// tools/kernel_resources.py: mix_copy_k 70 VGPRs, 7 waves a SIMD;
// mix_copy_huge_k 78 VGPRs, 6 waves a SIMD; no scratch, no LDS.  Occupancy
// does not bind either (8 KiB of loads in flight a wave), so the bounds come
// from trips, not from registers: tier 1 ends where a second trip would start,
// tier 2 where a reply's serial trips (16 x one memory round trip) pass the
// cost of a launch.  Measured (profiles/mixed_kernel_stats.md).
#include "zk_common.h"
#include "zk_mix.h"

namespace zk {

constexpr int MX_T = 256;
constexpr int MIX_G = 8;                      // lanes per tier-1 reply
constexpr int64_t MIX_SMALL = 256;            // tier 1 / 2 bound (bytes)
constexpr int64_t MIX_WAVE = 64 * 1024;       // tier 2 / 3 bound (bytes)
constexpr int MIX_HUGE_WG = 1024;             // workgroups on the tier-3 queue
constexpr int64_t MIX_CHUNK_U = 256;          // 16-byte units a tier-3 chunk
static_assert(MIX_SMALL == MIX_G * 16 * 2, "tier 1: one trip of two units");

// ---- split ------------------------------------------------------------------

__global__ __launch_bounds__(MX_T) void mix_class_k(
    const uint8_t* __restrict__ rx, const int64_t* __restrict__ foff,
    const int32_t* __restrict__ flen, const int64_t* __restrict__ n_dev,
    int64_t ncap, int32_t has_acl, int32_t* __restrict__ cls,
    int64_t* __restrict__ hist) {
  __shared__ int32_t h[MIX_CLASSES];
  if (threadIdx.x < MIX_CLASSES) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * MX_T + threadIdx.x;
  int32_t c = -1;
  if (i < ncap && i < *n_dev)
    c = mix_class(rx, foff[i], flen[i], has_acl != 0);
  if (i < ncap) cls[i] = c;
#pragma unroll
  for (int32_t k = 0; k < MIX_CLASSES; ++k) {
    const uint64_t m = __ballot(c == k);
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(&h[k], __popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < MIX_CLASSES)
    hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// mix_class_k under the second rule (zk_mix.h mix_class_setacl: opcode 7 to
// the ACL engine's class).  A kernel of its own text, so that mix_class_k
// stays the code it is for every caller that does not serve SET_ACL.
__global__ __launch_bounds__(MX_T) void mix_class_setacl_k(
    const uint8_t* __restrict__ rx, const int64_t* __restrict__ foff,
    const int32_t* __restrict__ flen, const int64_t* __restrict__ n_dev,
    int64_t ncap, int32_t has_acl, int32_t* __restrict__ cls,
    int64_t* __restrict__ hist) {
  __shared__ int32_t h[MIX_CLASSES];
  if (threadIdx.x < MIX_CLASSES) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * MX_T + threadIdx.x;
  int32_t c = -1;
  if (i < ncap && i < *n_dev)
    c = mix_class_setacl(rx, foff[i], flen[i], has_acl != 0);
  if (i < ncap) cls[i] = c;
#pragma unroll
  for (int32_t k = 0; k < MIX_CLASSES; ++k) {
    const uint64_t m = __ballot(c == k);
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(&h[k], __popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < MIX_CLASSES)
    hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// base: the exclusive scan of hist in class-major order (class c's run of
// block b starts at base[c * nblk + b], the class itself at base[c * nblk]).
__global__ __launch_bounds__(MX_T) void mix_scatter_k(
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    int64_t ncap, const int32_t* __restrict__ cls,
    const int64_t* __restrict__ base, const int64_t* __restrict__ total,
    int32_t* __restrict__ sub, int64_t* __restrict__ foff_c,
    int32_t* __restrict__ flen_c, int64_t* __restrict__ counts) {
  __shared__ int32_t cnt[MX_T / WAVE][MIX_CLASSES];
  const int64_t i = (int64_t)blockIdx.x * MX_T + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nblk = gridDim.x;
  if (blockIdx.x == 0 && threadIdx.x < MIX_CLASSES) {
    const int k = threadIdx.x;
    const int64_t b1 = k + 1 < MIX_CLASSES ? base[(int64_t)(k + 1) * nblk]
                                           : *total;
    counts[k] = b1 - base[(int64_t)k * nblk];
  }
  const int32_t c = i < ncap ? cls[i] : -1;
  const uint64_t below = (1ull << lane) - 1;
  int32_t r = 0;
#pragma unroll
  for (int32_t k = 0; k < MIX_CLASSES; ++k) {
    const uint64_t m = __ballot(c == k);
    if (c == k) r = __popcll(m & below);
    if (lane == 0) cnt[wv][k] = __popcll(m);
  }
  __syncthreads();
  if (i >= ncap) return;
  if (c < 0) {
    sub[i] = 0;
    return;
  }
  for (int k = 0; k < wv; ++k) r += cnt[k][c];
  const int64_t pos = base[(int64_t)c * nblk + blockIdx.x] -
                      base[(int64_t)c * nblk] + r;
  sub[i] = (int32_t)pos;
  foff_c[(int64_t)c * ncap + pos] = foff[i];
  flen_c[(int64_t)c * ncap + pos] = flen[i];
}

// ---- merge ------------------------------------------------------------------

struct MixSrc {                       // the three engines' outputs
  const uint8_t* stream[MIX_CLASSES];
  int64_t cap[MIX_CLASSES];           // bytes of each stream's buffer
  const int64_t* rec_off[MIX_CLASSES];
  const int64_t* total[MIX_CLASSES];
  const int32_t* err[MIX_CLASSES];
};

struct MixWs {
  int64_t* ctr;                 // [8] 0: nothing is written, 1: queued replies
  int64_t* sizes;               // [ncap] reply bytes
  int64_t* soff;                // [ncap] the reply's start in its stream
  int32_t* huge;                // [ncap] the tier-3 queue (request indices)
  int64_t* scan;                // zk_scan_workspace(ncap)
};

// (select chains, not indexed reads: the descriptor stays in scalar registers)
ZK_DEV const uint8_t* mix_stream(const MixSrc& s, int32_t c) {
  return c == 0 ? s.stream[0] : c == 1 ? s.stream[1] : s.stream[2];
}

// Sizes and source offsets.  A row the engines' outputs do not bear out (a
// class or index out of range, a span outside its stream) gets size 0: the
// copies stay in bounds whatever the tables hold.
__global__ __launch_bounds__(MX_T) void mix_size_k(
    const int32_t* __restrict__ cls, const int32_t* __restrict__ sub,
    const int64_t* __restrict__ n_dev, const int64_t* __restrict__ counts,
    int64_t ncap, MixSrc s, MixWs w) {
  const int64_t i = (int64_t)blockIdx.x * MX_T + threadIdx.x;
  if (i >= ncap) return;
  int64_t sz = 0, so = 0;
  if (i < *n_dev) {
    const int32_t c = cls[i];
    const int64_t j = sub[i];
    if (c >= 0 && c < MIX_CLASSES) {
      const int64_t nc = min(c == 0 ? counts[0] : c == 1 ? counts[1]
                                                          : counts[2], ncap);
      const int64_t* ro = c == 0 ? s.rec_off[0] : c == 1 ? s.rec_off[1]
                                                          : s.rec_off[2];
      const int64_t T = c == 0 ? *s.total[0] : c == 1 ? *s.total[1]
                                                      : *s.total[2];
      const int64_t cap = c == 0 ? s.cap[0] : c == 1 ? s.cap[1] : s.cap[2];
      if (j >= 0 && j < nc) {
        so = ro[j];
        const int64_t end = j + 1 < nc ? ro[j + 1] : T;
        sz = end - so;
        if (so < 0 || sz < 0 || end > cap || end > T) sz = 0;
      }
    }
  }
  w.sizes[i] = sz;
  w.soff[i] = so;
  if (sz > MIX_WAVE) {
    const unsigned long long k =
        atomicAdd((unsigned long long*)&w.ctr[1], 1ull);
    w.huge[k] = (int32_t)i;             // (at most one entry a request)
  }
}

// An engine's err is the merged one (the serve's first); otherwise 2 when
// the stream does not fit.  Either way the total is 0 and nothing is
// written.  The terminator, when it fits.
__global__ void mix_total_k(int64_t* __restrict__ total, int64_t out_cap,
                            int32_t* __restrict__ err, int32_t terminate,
                            uint8_t* __restrict__ out, MixSrc s, MixWs w) {
  const int64_t T = *total;
  int32_t e = *s.err[0];
  if (e == 0) e = *s.err[1];
  if (e == 0) e = *s.err[2];
  if (e == 0 && T > out_cap) e = 2;
  w.ctr[0] = e != 0 ? 1 : 0;
  *err = e;
  if (e != 0) *total = 0;
  if (e == 0 && terminate && T + 4 <= out_cap) st_be32(out + T, -1);
}

// 16 source bytes from byte `sh` of the aligned pair a | b.
ZK_DEV uint4 mix_realign(const uint4& a, const uint4& b, int sh) {
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const int ds = sh >> 2, bs = sh & 3;
  uint32_t t[5];
#pragma unroll
  for (int j = 0; j < 5; ++j)
    t[j] = ds == 0 ? w[j] : ds == 1 ? w[j + 1] : ds == 2 ? w[j + 2]
                                                           : w[j + 3];
  uint4 v;
  v.x = __builtin_amdgcn_alignbyte(t[1], t[0], bs);
  v.y = __builtin_amdgcn_alignbyte(t[2], t[1], bs);
  v.z = __builtin_amdgcn_alignbyte(t[3], t[2], bs);
  v.w = __builtin_amdgcn_alignbyte(t[4], t[3], bs);
  return v;
}

// 16-byte units [k0, k1) of sb -> db (db 16-byte aligned, sb anywhere) by the
// nt lanes of a team (this lane is t): U units a lane a trip, their loads
// before the first store.  The aligned word holding a unit's first byte and,
// for a source across two words, the next one (which holds the unit's last
// byte): no load leaves the 16-byte words the span touches.
template <int U>
ZK_DEV void mix_units(uint8_t* __restrict__ db, const uint8_t* __restrict__ sb,
                      int64_t k0, int64_t k1, int t, int nt) {
  const int sh = (int)((uintptr_t)sb & 15);
  const uint4* sa = (const uint4*)((uintptr_t)sb & ~(uintptr_t)15);
  for (int64_t k = k0 + t; k < k1; k += (int64_t)nt * U) {
    uint4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kk = k + (int64_t)u * nt;
      a[u] = b[u] = make_uint4(0, 0, 0, 0);
      if (kk < k1) {
        a[u] = sa[kk];
        if (sh != 0) b[u] = sa[kk + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kk = k + (int64_t)u * nt;
      if (kk < k1) *(uint4*)(db + 16 * kk) = mix_realign(a[u], b[u], sh);
    }
  }
}

// The span of one reply: the bytes before the destination's first 16-byte
// boundary, the aligned units, the bytes after the last.
struct MixSpan {
  int64_t head, units, tail0;
};
ZK_DEV MixSpan mix_span(const uint8_t* d, int64_t n) {
  int64_t head = (16 - (int64_t)((uintptr_t)d & 15)) & 15;
  if (head > n) head = n;
  const int64_t units = (n - head) >> 4;
  return MixSpan{head, units, head + 16 * units};
}

ZK_DEV void mix_edges(uint8_t* __restrict__ d, const uint8_t* __restrict__ s,
                      int64_t n, const MixSpan& p, int t, int nt) {
  for (int64_t b = t; b < p.head; b += nt) d[b] = s[b];
  for (int64_t b = p.tail0 + t; b < n; b += nt) d[b] = s[b];
}

// Tiers 1 and 2.  MIX_G lanes a request; then the wave takes its (at most 8)
// requests of tier 2 one at a time with all its lanes.  (A launch of a wave
// per request for tier 2 cost 114 us per 1M requests to find nothing to do.)
__global__ __launch_bounds__(MX_T) void mix_copy_k(
    const int32_t* __restrict__ cls, const int64_t* __restrict__ n_dev,
    int64_t ncap, MixSrc s, MixWs w, const int64_t* __restrict__ rec_off,
    uint8_t* __restrict__ out) {
  if (w.ctr[0] != 0) return;                        // (grid-uniform)
  const int64_t g = (int64_t)blockIdx.x * MX_T + threadIdx.x;
  const int64_t i = g / MIX_G;
  const int l = (int)(g % MIX_G);
  const int lane = threadIdx.x & 63;
  int64_t n = 0;
  const uint8_t* src = nullptr;
  uint8_t* d = nullptr;
  if (i < ncap && i < *n_dev) {
    n = w.sizes[i];
    if (n > 0 && n <= MIX_WAVE) {
      src = mix_stream(s, cls[i]) + w.soff[i];
      d = out + rec_off[i];
    }
  }
  if (n > 0 && n <= MIX_SMALL) {
    const MixSpan p = mix_span(d, n);
    mix_units<2>(d + p.head, src + p.head, 0, p.units, l, MIX_G);
    mix_edges(d, src, n, p, l, MIX_G);
  }
  uint64_t todo = __ballot(l == 0 && n > MIX_SMALL && n <= MIX_WAVE);
  while (todo != 0) {                               // (wave-uniform)
    const int first = __ffsll((unsigned long long)todo) - 1;
    const int64_t n2 = __shfl(n, first, 64);
    const uint8_t* s2 = (const uint8_t*)__shfl((int64_t)(uintptr_t)src, first,
                                               64);
    uint8_t* d2 = (uint8_t*)__shfl((int64_t)(uintptr_t)d, first, 64);
    const MixSpan p = mix_span(d2, n2);
    mix_units<4>(d2 + p.head, s2 + p.head, 0, p.units, lane, 64);
    mix_edges(d2, s2, n2, p, lane, 64);
    todo &= todo - 1;
  }
}

// Tier 3: the queue mix_size_k filled.  The MIX_HUGE_WG workgroups' waves
// form min(nq, NW) groups, a group takes an entry at a time and its G waves
// the entry's chunks in turn: a wave reads the rows of the entries of its
// group only (every wave walking the whole queue paid a dependent round trip
// per entry: 1.3 TB/s on 64 replies of 4 MiB, 1.9 TB/s so).
__global__ __launch_bounds__(MX_T) void mix_copy_huge_k(
    const int32_t* __restrict__ cls, int64_t ncap, MixSrc s, MixWs w,
    const int64_t* __restrict__ rec_off, uint8_t* __restrict__ out) {
  if (w.ctr[0] != 0) return;                        // (grid-uniform)
  const int64_t nq = min(w.ctr[1], ncap);
  if (nq <= 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * (MX_T / 64) + (threadIdx.x >> 6);
  constexpr int64_t NW = (int64_t)MIX_HUGE_WG * (MX_T / 64);
  const int64_t ng = min(nq, NW);
  const int64_t G = NW / ng;
  const int64_t grp = gw / G, gl = gw % G;
  if (grp >= ng) return;
  for (int64_t e = grp; e < nq; e += ng) {
    const int64_t i = w.huge[e];
    if (i < 0 || i >= ncap) continue;
    const int64_t n = w.sizes[i];
    const uint8_t* src = mix_stream(s, cls[i]) + w.soff[i];
    uint8_t* d = out + rec_off[i];
    const MixSpan p = mix_span(d, n);
    for (int64_t c = gl; c * MIX_CHUNK_U < p.units; c += G) {
      const int64_t k0 = c * MIX_CHUNK_U;
      mix_units<4>(d + p.head, src + p.head, k0,
                   min(k0 + MIX_CHUNK_U, p.units), lane, 64);
    }
    if (gl == 0) mix_edges(d, src, n, p, lane, 64);
  }
}

}  // namespace zk

extern "C" {

int64_t zk_tree_mix_small(void) { return zk::MIX_SMALL; }
int64_t zk_tree_mix_wave(void) { return zk::MIX_WAVE; }

static int64_t mix_a16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// Bytes of zk_tree_mix_split's workspace for ncap frames: the histogram, its
// scan, the scan's total and workspace.  Nothing in it needs zeroing.
int64_t zk_tree_mix_split_workspace(int64_t ncap) {
  if (ncap < 0) ncap = 0;
  const int64_t nblk = (ncap + zk::MX_T - 1) / zk::MX_T;
  const int64_t m = zk::MIX_CLASSES * nblk;
  return mix_a16(8 * (2 * m + 8 + zk_scan_workspace(m > 0 ? m : 1)));
}

// Split the frame table (foff / flen, *n_dev frames, at most ncap) of rx by
// engine class: cls[ncap] (-1 past *n_dev), sub[ncap] (the frame's index in
// its class), the compacted tables foff_c / flen_c ([3][ncap], class c's at
// c * ncap) and counts[3].  Stable.  has_acl: the tree keeps an ACL table.
// setacl: the second rule (zk_mix.h mix_class_setacl), the same launches.
static int mix_split_launch(const uint8_t* rx, const int64_t* foff,
                            const int32_t* flen, const int64_t* n_dev,
                            int64_t ncap, int32_t has_acl, int32_t setacl,
                            int32_t* cls, int32_t* sub, int64_t* foff_c,
                            int32_t* flen_c, int64_t* counts, uint8_t* ws,
                            int64_t ws_bytes, hipStream_t st) {
  if (ncap <= 0)
    return hipMemsetAsync(counts, 0, sizeof(int64_t) * zk::MIX_CLASSES, st) !=
                   hipSuccess ? -4 : 0;
  if (ncap >= 0x7fffffff) return -1;               // sub[]: int32
  if (ws_bytes < zk_tree_mix_split_workspace(ncap) || ((uintptr_t)ws & 15))
    return -1;
  const int64_t nblk = (ncap + zk::MX_T - 1) / zk::MX_T;
  const int64_t m = zk::MIX_CLASSES * nblk;
  int64_t* hist = (int64_t*)ws;
  int64_t* base = hist + m;
  int64_t* total = hist + 2 * m;
  int64_t* sws = hist + 2 * m + 8;
  if (setacl)
    zk::mix_class_setacl_k<<<(unsigned)nblk, zk::MX_T, 0, st>>>(
        rx, foff, flen, n_dev, ncap, has_acl, cls, hist);
  else
    zk::mix_class_k<<<(unsigned)nblk, zk::MX_T, 0, st>>>(
        rx, foff, flen, n_dev, ncap, has_acl, cls, hist);
  ZK_LAUNCH_CHECK();
  const int rc = zk_scan_excl_i64(hist, base, m, total, sws, st);
  if (rc) return rc;
  zk::mix_scatter_k<<<(unsigned)nblk, zk::MX_T, 0, st>>>(
      foff, flen, ncap, cls, base, total, sub, foff_c, flen_c, counts);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_tree_mix_split(const uint8_t* rx, const int64_t* foff,
                      const int32_t* flen, const int64_t* n_dev, int64_t ncap,
                      int32_t has_acl, int32_t* cls, int32_t* sub,
                      int64_t* foff_c, int32_t* flen_c, int64_t* counts,
                      uint8_t* ws, int64_t ws_bytes, hipStream_t st) {
  return mix_split_launch(rx, foff, flen, n_dev, ncap, has_acl, 0, cls, sub,
                          foff_c, flen_c, counts, ws, ws_bytes, st);
}

// zk_tree_mix_split for a caller that serves SET_ACL: opcode 7 goes to the
// ACL engine's class (on a tree with an ACL table).
int zk_tree_mix_split_setacl(const uint8_t* rx, const int64_t* foff,
                             const int32_t* flen, const int64_t* n_dev,
                             int64_t ncap, int32_t has_acl, int32_t* cls,
                             int32_t* sub, int64_t* foff_c, int32_t* flen_c,
                             int64_t* counts, uint8_t* ws, int64_t ws_bytes,
                             hipStream_t st) {
  return mix_split_launch(rx, foff, flen, n_dev, ncap, has_acl, 1, cls, sub,
                          foff_c, flen_c, counts, ws, ws_bytes, st);
}

static int64_t mix_merge_layout(int64_t ncap, uint8_t* ws, zk::MixWs* w) {
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    uint8_t* p = ws != nullptr ? ws + o : nullptr;
    o += mix_a16(bytes);
    return p;
  };
  uint8_t* ctr = take(64);
  uint8_t* sizes = take(ncap * 8);
  uint8_t* soff = take(ncap * 8);
  uint8_t* huge = take(ncap * 4);
  uint8_t* scan = take(zk_scan_workspace(ncap > 0 ? ncap : 1) * 8);
  if (w != nullptr) {
    w->ctr = (int64_t*)ctr;
    w->sizes = (int64_t*)sizes;
    w->soff = (int64_t*)soff;
    w->huge = (int32_t*)huge;
    w->scan = (int64_t*)scan;
  }
  return o;
}

// Bytes of zk_tree_mix_merge's workspace for ncap requests (16-aligned
// parts).  Nothing in it needs zeroing.
int64_t zk_tree_mix_merge_workspace(int64_t ncap) {
  return mix_merge_layout(ncap > 0 ? ncap : 0, nullptr, nullptr);
}

// Merge the three engines' reply streams into request order: request i (of
// *n_dev, at most ncap) takes reply sub[i] of stream cls[i] (stream c:
// counts[c] replies starting at rec_off_c[], *total_c bytes in a buffer of
// cap_c, its encoder's *err_c) -> out[0, *total), the starts -> rec_off[ncap].
// A non-zero err_c is the merged *err (class 0 first), else 2 when the stream
// does not fit out_cap; then *total = 0 and nothing is written.
int zk_tree_mix_merge(const int32_t* cls, const int32_t* sub,
                      const int64_t* n_dev, const int64_t* counts,
                      int64_t ncap, const uint8_t* const* stream,
                      const int64_t* stream_cap,
                      const int64_t* const* rec_off_c,
                      const int64_t* const* total_c,
                      const int32_t* const* err_c, uint8_t* ws,
                      int64_t ws_bytes, uint8_t* out, int64_t out_cap,
                      int64_t* rec_off, int64_t* total, int32_t* err,
                      int32_t terminate, hipStream_t st) {
  if (out_cap < 0) return -1;
  if (ncap <= 0) {
    if (hipMemsetAsync(total, 0, sizeof(int64_t), st) != hipSuccess) return -4;
    if (hipMemsetAsync(err, 0, sizeof(int32_t), st) != hipSuccess) return -4;
    if (terminate && out_cap >= 4 &&
        hipMemsetAsync(out, 0xFF, 4, st) != hipSuccess)
      return -4;
    return 0;
  }
  if (ncap >= (int64_t)0x7fffffff / zk::MIX_G) return -1;
  if (ws_bytes < zk_tree_mix_merge_workspace(ncap) || ((uintptr_t)ws & 15))
    return -1;
  zk::MixWs w;
  mix_merge_layout(ncap, ws, &w);
  zk::MixSrc s;
  for (int c = 0; c < zk::MIX_CLASSES; ++c) {
    if (stream_cap[c] < 0) return -1;
    s.stream[c] = stream[c];
    s.cap[c] = stream_cap[c];
    s.rec_off[c] = rec_off_c[c];
    s.total[c] = total_c[c];
    s.err[c] = err_c[c];
  }
  if (hipMemsetAsync(w.ctr, 0, 64, st) != hipSuccess) return -4;
  const unsigned nb = (unsigned)((ncap + zk::MX_T - 1) / zk::MX_T);
  zk::mix_size_k<<<nb, zk::MX_T, 0, st>>>(cls, sub, n_dev, counts, ncap, s, w);
  ZK_LAUNCH_CHECK();
  const int rc = zk_scan_excl_i64(w.sizes, rec_off, ncap, total, w.scan, st);
  if (rc) return rc;
  zk::mix_total_k<<<1, 1, 0, st>>>(total, out_cap, err, terminate, out, s, w);
  ZK_LAUNCH_CHECK();
  const unsigned nbs =
      (unsigned)((ncap * zk::MIX_G + zk::MX_T - 1) / zk::MX_T);
  zk::mix_copy_k<<<nbs, zk::MX_T, 0, st>>>(cls, n_dev, ncap, s, w, rec_off,
                                           out);
  ZK_LAUNCH_CHECK();
  zk::mix_copy_huge_k<<<zk::MIX_HUGE_WG, zk::MX_T, 0, st>>>(cls, ncap, s, w,
                                                            rec_off, out);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
