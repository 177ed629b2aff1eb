// The front end's device-side I/O staging (zkmi/server/gpu.py GpuZKServer;
// the rules: zk_front.h).  A tick of the front end uploads what every
// connection has received, byte for byte, as one raw stream with a segment per
// connection, serves it as one session batch and sends every connection its
// bytes.  Two problems on either side of the serve are solved here, with no
// host read, no atomics and no lane that waits for another:
//
// The cut (before the serve; a session batch refuses a torn frame for
// everyone):
//   front_table_k   a lane per boundary of raw_starts: front_boundary_bad; an
//                   unsound table sets the fault word and nothing is taken
//   front_cut_k     a wave per segment: front_walk over the segment, staged
//                   through LDS a chunk of FC_CHUNK bytes at a time.  The
//                   walk's state is wave-uniform (scalars); a word it asks for
//                   outside the staged window moves the window to that word,
//                   so a length or an opcode word that straddles a chunk is
//                   read whole from the next one, and a long body is skipped,
//                   not staged.  -> take[s], nfr[s], flag[s]
//                   (front_cut_k<true>: front_walk_ordered, the cut in front of
//                   the ordered session serve, and nwr[s]; the phase is one
//                   more word of that state)
//   (the device-wide scan of take[]: starts[S + 1] of the session batch)
//   front_gather_k  the taken prefixes packed into the dense rx
//
// The TX assembly (after the serve; a connection's bytes are scattered over
// the reply stream and three notification streams):
//   front_owner_k   one workgroup: the 64-entry owner table of the watcher
//                   slots (the lowest-numbered segment naming a slot) and the
//                   count of segments that name a slot another one owns
//   front_pieces_k  a lane per connection: its four piece descriptors
//                   (stream, offset, length), in sending order
//                   (front_pieces_k<true>: the replies end at rep_end[s], the
//                   ordered serve's deferral)
//   (the device-wide scan of the lengths: tx_off and the total)
//   front_gather_k  the same kernel: the pieces into one TX buffer
//
// front_gather_k: a lane per 16 aligned destination bytes finds its piece by
// binary search over the scanned offsets, so the work is balanced and the
// stores coalesced whether a piece is 20 bytes or 1 MiB.  A unit that lies
// inside one piece is one 16-byte store of the source realigned in registers
// (tree_mix.hip mix_copy_k's way: the aligned word holding the unit's first
// source byte and, for a source across two words, the next one); a unit that
// holds a piece boundary or the stream's end is copied byte by byte.
#include "zk_common.h"
#include "zk_front.h"

namespace zk {

constexpr int FC_T = 64;                 // front_cut_k: a wave a workgroup
constexpr int FC_CHUNK = 4096;           // bytes of the staged window
constexpr int FC_U = FC_CHUNK / (16 * FC_T);
static_assert(FC_U * 16 * FC_T == FC_CHUNK, "whole 16-byte units a lane");
constexpr int FG_T = 256;
constexpr int FG_MAX_WG = 2048;

__global__ __launch_bounds__(FG_T) void front_table_k(
    const int64_t* __restrict__ raw_starts, int64_t S, int64_t n,
    int64_t* __restrict__ fault) {
  const int64_t s = (int64_t)blockIdx.x * FG_T + threadIdx.x;
  if (s > S) return;
  // (every lane that finds one writes the same word the same value)
  if (front_boundary_bad(raw_starts, S, n, s) != 0) *fault = 1;
}

// 16 bytes of raw at p (raw + p is 16-byte aligned): one vector load where
// they lie inside [0, end), byte loads of the ones that do at the two ends,
// zeros elsewhere.  end <= the stream's length.
ZK_DEV uint4 fc_fetch(const uint8_t* __restrict__ raw, int64_t p, int64_t end) {
  uint4 v = {0u, 0u, 0u, 0u};
  if (p >= end || p + 16 <= 0) return v;
  if (p >= 0 && p + 16 <= end) return *reinterpret_cast<const uint4*>(raw + p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (int i = 0; i < 16; ++i) {
    const int64_t q = p + i;
    if (q >= 0 && q < end) w[i >> 2] |= (uint32_t)raw[q] << (8 * (i & 3));
  }
  v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
  return v;
}

// ORD: front_walk_ordered (has_acl: zk_mix.h's class rule) and nwr[s], the
// write frames taken; the plain instance reads neither.
template <bool ORD>
__global__ __launch_bounds__(FC_T) void front_cut_k(
    const uint8_t* __restrict__ raw, int64_t n, int64_t raw_mis,
    const int64_t* __restrict__ raw_starts, int64_t S, int64_t quota,
    int64_t max_packet, const int64_t* __restrict__ fault,
    int64_t* __restrict__ take, int32_t* __restrict__ nfr,
    int32_t* __restrict__ flag, int32_t has_acl, int32_t* __restrict__ nwr) {
  // (one word past the window: the high half of the last word's pair)
  __shared__ __attribute__((aligned(16))) uint32_t win[FC_CHUNK / 4 + 4];
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  if (s >= S) return;
  // the segment [a, b), clipped to the stream whatever the table holds
  int64_t a = 0, b = 0;
  if (*fault == 0) {
    a = raw_starts[s];
    b = raw_starts[s + 1];
    if (a < 0) a = 0;
    if (b > n) b = n;
    if (b < a) b = a;
  }
  FrontCut c{0, 0, 0};
  int32_t wr = 0;                        // (ORD)
  if (b - a >= 4) {                      // (else: the wave leaves at once)
    // everything of the walk is wave-uniform: the window's base included
    int64_t wb = -((int64_t)1 << 62);    // no window yet
    auto rd = [&](int64_t p) -> int32_t {
      const int64_t q = a + p;           // [q, q + 4) lies inside [a, b)
      if (q < wb || q + 4 > wb + FC_CHUNK) {
        __syncthreads();                 // the reads of the old window are done
        wb = ((q + raw_mis) & ~(int64_t)15) - raw_mis;
#pragma unroll
        for (int u = 0; u < FC_U; ++u) {
          const int k = lane + u * FC_T;
          *reinterpret_cast<uint4*>(&win[4 * k]) =
              fc_fetch(raw, wb + 16 * (int64_t)k, b);
        }
        __syncthreads();
      }
      const uint32_t r = (uint32_t)(q - wb);
      const uint32_t i = r >> 2;
      const uint64_t two = ((uint64_t)win[i + 1] << 32) | win[i];
      // (every lane read the same word: as a scalar the walk's state stays in
      // SGPRs and its branches are the scalar unit's)
      return __builtin_amdgcn_readfirstlane(
          (int32_t)bswap32((uint32_t)(two >> (8 * (r & 3)))));
    };
    if (ORD) {
      const FrontCutOrd o =
          front_walk_ordered(b - a, quota, max_packet, has_acl != 0, rd);
      c.take = o.take, c.nfr = o.nfr, c.flag = o.flag;
      wr = o.nwr;
    } else {
      c = front_walk(b - a, quota, max_packet, rd);
    }
  }
  if (lane == 0) {
    take[s] = c.take;
    nfr[s] = c.nfr;
    flag[s] = c.flag;
    if (ORD) nwr[s] = wr;
  }
}

// front_cut_k in front of a serve that takes SET_ACL (zk_front.h
// front_walk_setacl / front_walk_ordered_setacl: such a frame is a run of its
// own).  Kernels of their own text: front_cut_k's two instances stay the code
// they are.
template <bool ORD>
__global__ __launch_bounds__(FC_T) void front_cut_setacl_k(
    const uint8_t* __restrict__ raw, int64_t n, int64_t raw_mis,
    const int64_t* __restrict__ raw_starts, int64_t S, int64_t quota,
    int64_t max_packet, const int64_t* __restrict__ fault,
    int64_t* __restrict__ take, int32_t* __restrict__ nfr,
    int32_t* __restrict__ flag, int32_t has_acl, int32_t* __restrict__ nwr) {
  // (one word past the window: the high half of the last word's pair)
  __shared__ __attribute__((aligned(16))) uint32_t win[FC_CHUNK / 4 + 4];
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  if (s >= S) return;
  // the segment [a, b), clipped to the stream whatever the table holds
  int64_t a = 0, b = 0;
  if (*fault == 0) {
    a = raw_starts[s];
    b = raw_starts[s + 1];
    if (a < 0) a = 0;
    if (b > n) b = n;
    if (b < a) b = a;
  }
  FrontCut c{0, 0, 0};
  int32_t wr = 0;                        // (ORD)
  if (b - a >= 4) {                      // (else: the wave leaves at once)
    // everything of the walk is wave-uniform: the window's base included
    int64_t wb = -((int64_t)1 << 62);    // no window yet
    auto rd = [&](int64_t p) -> int32_t {
      const int64_t q = a + p;           // [q, q + 4) lies inside [a, b)
      if (q < wb || q + 4 > wb + FC_CHUNK) {
        __syncthreads();                 // the reads of the old window are done
        wb = ((q + raw_mis) & ~(int64_t)15) - raw_mis;
#pragma unroll
        for (int u = 0; u < FC_U; ++u) {
          const int k = lane + u * FC_T;
          *reinterpret_cast<uint4*>(&win[4 * k]) =
              fc_fetch(raw, wb + 16 * (int64_t)k, b);
        }
        __syncthreads();
      }
      const uint32_t r = (uint32_t)(q - wb);
      const uint32_t i = r >> 2;
      const uint64_t two = ((uint64_t)win[i + 1] << 32) | win[i];
      // (every lane read the same word: as a scalar the walk's state stays in
      // SGPRs and its branches are the scalar unit's)
      return __builtin_amdgcn_readfirstlane(
          (int32_t)bswap32((uint32_t)(two >> (8 * (r & 3)))));
    };
    if (ORD) {
      const FrontCutOrd o =
          front_walk_ordered_setacl(b - a, quota, max_packet, has_acl != 0, rd);
      c.take = o.take, c.nfr = o.nfr, c.flag = o.flag;
      wr = o.nwr;
    } else {
      c = front_walk_setacl(b - a, quota, max_packet, rd);
    }
  }
  if (lane == 0) {
    take[s] = c.take;
    nfr[s] = c.nfr;
    flag[s] = c.flag;
    if (ORD) nwr[s] = wr;
  }
}

// The streams a gather reads.
struct FrontSrc {
  const uint8_t* p[FRONT_PIECES];
  int64_t cap[FRONT_PIECES];
};

// 16 source bytes from byte `sh` of the aligned pair a | b (mix_realign).
ZK_DEV uint4 fg_realign(const uint4& a, const uint4& b, int sh) {
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

// Where piece i's bytes are, or null when its descriptor does not lie inside
// its stream (such a piece is not copied).
ZK_DEV const uint8_t* fg_source(const FrontSrc& src,
                                const int32_t* __restrict__ p_stream,
                                const int64_t* __restrict__ p_src,
                                const int64_t* __restrict__ p_off, int64_t i) {
  const int32_t st = p_stream != nullptr ? p_stream[i] : 0;
  if (st < 0 || st >= FRONT_PIECES) return nullptr;
  const uint8_t* base = st == 0 ? src.p[0] : st == 1 ? src.p[1]
                        : st == 2 ? src.p[2] : src.p[3];
  const int64_t cap = st == 0 ? src.cap[0] : st == 1 ? src.cap[1]
                      : st == 2 ? src.cap[2] : src.cap[3];
  const int64_t so = p_src[i];
  const int64_t len = p_off[i + 1] - p_off[i];
  if (base == nullptr || so < 0 || len < 0 || so > cap || len > cap - so)
    return nullptr;
  return base + so;
}

// Piece i (source p_src[i] of stream p_stream[i], or stream 0 without the
// table) -> dst[p_off[i], p_off[i + 1]), i < P; the total p_off[P].  A total
// past dst_cap writes nothing and sets *over.  dmis: dst's address mod 16.
__global__ __launch_bounds__(FG_T) void front_gather_k(
    FrontSrc src, const int32_t* __restrict__ p_stream,
    const int64_t* __restrict__ p_src, const int64_t* __restrict__ p_off,
    int64_t P, uint8_t* __restrict__ dst, int64_t dst_cap, int64_t dmis,
    int64_t* __restrict__ over) {
  const int64_t g = (int64_t)blockIdx.x * FG_T + threadIdx.x;
  const int64_t total = p_off[P];
  const bool ov = total < 0 || total > dst_cap;
  if (g == 0) *over = ov ? 1 : 0;
  if (ov) return;                                   // (grid-uniform)
  // unit k: the aligned 16 bytes dst[16 k - dmis, 16 k - dmis + 16)
  const int64_t units = (total + dmis + 15) >> 4;
  for (int64_t k = g; k < units; k += (int64_t)gridDim.x * FG_T) {
    const int64_t d0 = 16 * k - dmis, d1 = d0 + 16;
    const int64_t lo = d0 < 0 ? 0 : d0, hi = d1 > total ? total : d1;
    if (lo >= hi) continue;
    int64_t i = front_piece_at(p_off, P, lo);
    if (lo == d0 && hi == d1 && p_off[i] <= d0 && p_off[i + 1] >= d1) {
      const uint8_t* sb = fg_source(src, p_stream, p_src, p_off, i);
      if (sb == nullptr) continue;
      sb += d0 - p_off[i];
      const int sh = (int)((uintptr_t)sb & 15);
      const uint4* sa = (const uint4*)((uintptr_t)sb & ~(uintptr_t)15);
      const uint4 a = sa[0];
      uint4 b = make_uint4(0, 0, 0, 0);
      if (sh != 0) b = sa[1];
      *reinterpret_cast<uint4*>(dst + d0) = fg_realign(a, b, sh);
      continue;
    }
    // an edge: a piece boundary or the stream's end inside the unit
    for (int64_t d = lo; d < hi; ++d) {
      while (i + 1 < P && p_off[i + 1] <= d) ++i;
      if (d < p_off[i] || d >= p_off[i + 1]) continue;
      const uint8_t* sb = fg_source(src, p_stream, p_src, p_off, i);
      if (sb != nullptr) dst[d] = sb[d - p_off[i]];
    }
  }
}

// stats[]: what GpuZKServer.stats reports of the assembly
enum : int { FTS_DUP = 0, FTS_N = 8 };

__global__ __launch_bounds__(FG_T) void front_owner_k(
    const int32_t* __restrict__ wslots, int64_t S, int64_t* __restrict__ owner,
    int64_t* __restrict__ stats) {
  __shared__ int32_t chunk[FG_T];
  const int t = threadIdx.x;
  int64_t own = -1, named = 0;
  for (int64_t base = 0; base < S; base += FG_T) {
    chunk[t] = base + t < S ? wslots[base + t] : -1;
    __syncthreads();
    const int64_t cnt = S - base < FG_T ? S - base : FG_T;
    if (t < FRONT_SLOTS) front_owner_scan(chunk, cnt, base, t, own, named);
    __syncthreads();
  }
  if (t >= FRONT_SLOTS) return;                     // (wave 0 is whole)
  owner[t] = own;
  int64_t dup = named > 1 ? named - 1 : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) dup += __shfl_xor(dup, d, 64);
  if (t == 0) stats[FTS_DUP] = dup;
}

// END: t.rep_end ends the reply pieces; the plain instance does not read it.
template <bool END>
__global__ __launch_bounds__(FG_T) void front_pieces_k(
    FrontTx t, int32_t* __restrict__ p_stream, int64_t* __restrict__ p_src,
    int64_t* __restrict__ p_len) {
  const int64_t s = (int64_t)blockIdx.x * FG_T + threadIdx.x;
  if (s >= t.S) return;
#pragma unroll
  for (int k = 0; k < FRONT_PIECES; ++k) {
    const FrontPiece p = front_piece<END>(t, s, k);
    p_stream[FRONT_PIECES * s + k] = p.stream;
    p_src[FRONT_PIECES * s + k] = p.src;
    p_len[FRONT_PIECES * s + k] = p.len;
  }
}

static_assert(FRONT_SLOTS == WAVE, "front_owner_k: a lane a slot, one wave");

static unsigned fg_blocks(int64_t n) {
  return (unsigned)((n + FG_T - 1) / FG_T);
}

}  // namespace zk

extern "C" {

// Bytes of front_cut_k's staged window: a word of a segment that straddles a
// multiple of it (from the segment's first 16-byte boundary) is read from a
// window of its own.
int64_t zk_front_chunk(void) { return zk::FC_CHUNK; }

// The cut.  raw[0, n) with raw_starts[S + 1] (segment s: raw[raw_starts[s],
// raw_starts[s + 1])), at most `quota` frames a segment, K1's max_packet ->
// take[S] (bytes to serve), nfr[S] (frames in them), flag[S] (1: bad length)
// and fault[1] (1: the table is unsound; then every take is 0).
// mode 0: front_walk.  mode 1: front_walk_ordered, with has_acl (the tree
// keeps an ACL table: GET_ACL is of the ACL engine's class) -> nwr[S] too, the
// write frames taken (mode 0 takes nwr null and leaves it alone).  mode 2 /
// mode 3: modes 0 / 1 in front of a serve that takes SET_ACL (zk_front.h
// front_walk_setacl / front_walk_ordered_setacl).
int zk_front_cut_mode(const uint8_t* raw, int64_t n, const int64_t* raw_starts,
                      int64_t S, int64_t quota, int64_t max_packet,
                      int32_t mode, int32_t has_acl, int64_t* take,
                      int32_t* nfr, int32_t* flag, int32_t* nwr,
                      int64_t* fault, hipStream_t st) {
  if (S < 1 || S > 0x7fffffff || n < 0 || max_packet < 0 || mode < 0 ||
      mode > 3 || ((mode & 1) && nwr == nullptr))
    return (int)hipErrorInvalidValue;
  if (hipMemsetAsync(fault, 0, sizeof(int64_t), st) != hipSuccess) return -4;
  zk::front_table_k<<<zk::fg_blocks(S + 1), zk::FG_T, 0, st>>>(raw_starts, S,
                                                               n, fault);
  ZK_LAUNCH_CHECK();
  if (mode == 3)
    zk::front_cut_setacl_k<true><<<(unsigned)S, zk::FC_T, 0, st>>>(
        raw, n, (int64_t)((uintptr_t)raw & 15), raw_starts, S, quota,
        max_packet, fault, take, nfr, flag, has_acl, nwr);
  else if (mode == 2)
    zk::front_cut_setacl_k<false><<<(unsigned)S, zk::FC_T, 0, st>>>(
        raw, n, (int64_t)((uintptr_t)raw & 15), raw_starts, S, quota,
        max_packet, fault, take, nfr, flag, 0, nullptr);
  else if (mode == 1)
    zk::front_cut_k<true><<<(unsigned)S, zk::FC_T, 0, st>>>(
        raw, n, (int64_t)((uintptr_t)raw & 15), raw_starts, S, quota,
        max_packet, fault, take, nfr, flag, has_acl, nwr);
  else
    zk::front_cut_k<false><<<(unsigned)S, zk::FC_T, 0, st>>>(
        raw, n, (int64_t)((uintptr_t)raw & 15), raw_starts, S, quota,
        max_packet, fault, take, nfr, flag, 0, nullptr);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_front_cut(const uint8_t* raw, int64_t n, const int64_t* raw_starts,
                 int64_t S, int64_t quota, int64_t max_packet, int64_t* take,
                 int32_t* nfr, int32_t* flag, int64_t* fault, hipStream_t st) {
  return zk_front_cut_mode(raw, n, raw_starts, S, quota, max_packet, 0, 0, take,
                           nfr, flag, nullptr, fault, st);
}

// The gather.  streams[4] / caps[4] (host arrays; a null stream has no
// pieces), piece i < P: p_off[i + 1] - p_off[i] bytes at p_src[i] of stream
// p_stream[i] (null: stream 0) -> dst[p_off[i], ...); p_off[P + 1] is the
// scan of the lengths.  over[1]: 1 when p_off[P] > dst_cap (nothing written).
int zk_front_gather(const uint8_t* const* streams, const int64_t* caps,
                    const int32_t* p_stream, const int64_t* p_src,
                    const int64_t* p_off, int64_t P, uint8_t* dst,
                    int64_t dst_cap, int64_t* over, hipStream_t st) {
  if (P < 1 || P > 0x7fffffff || dst_cap < 0) return (int)hipErrorInvalidValue;
  zk::FrontSrc src;
  for (int k = 0; k < zk::FRONT_PIECES; ++k) {
    src.p[k] = streams[k];
    src.cap[k] = streams[k] != nullptr && caps[k] > 0 ? caps[k] : 0;
  }
  const int64_t units = (dst_cap + 15) / 16 + 1;
  int64_t nb = (units + zk::FG_T - 1) / zk::FG_T;
  if (nb > zk::FG_MAX_WG) nb = zk::FG_MAX_WG;
  zk::front_gather_k<<<(unsigned)nb, zk::FG_T, 0, st>>>(
      src, p_stream, p_src, p_off, P, dst, dst_cap,
      (int64_t)((uintptr_t)dst & 15), over);
  ZK_LAUNCH_CHECK();
  return 0;
}

// The TX pieces.  rep_off[S + 1] (or null), wslots[S], slot_off[3] (host
// array of device tables [65], each or all null: the catch-up, write-fired
// and close-fired notification streams), the batch's err word (or null),
// caps[4] (host array: the four streams' bytes), owner[64] (workspace) ->
// piece 4 s + k of connection s (p_stream / p_src / p_len [4 S]) and
// stats[8]: [0] the segments that name a watcher slot another one owns.
// rep_end[S] (or null): connection s's replies end there instead of at
// rep_off[s + 1] (the ordered serve's deferral).
int zk_front_tx_pieces_end(const int64_t* rep_off, const int64_t* rep_end,
                           const int32_t* wslots,
                           const int64_t* const* slot_off, const int32_t* err,
                           const int64_t* caps, int64_t S, int64_t* owner,
                           int32_t* p_stream, int64_t* p_src, int64_t* p_len,
                           int64_t* stats, hipStream_t st) {
  if (S < 1 || S > 0x1fffffff) return (int)hipErrorInvalidValue;
  zk::front_owner_k<<<1, zk::FG_T, 0, st>>>(wslots, S, owner, stats);
  ZK_LAUNCH_CHECK();
  zk::FrontTx t;
  t.rep_off = rep_off;
  for (int k = 0; k < 3; ++k) t.slot_off[k] = slot_off[k];
  for (int k = 0; k < zk::FRONT_PIECES; ++k) t.cap[k] = caps[k] > 0 ? caps[k] : 0;
  t.err = err;
  t.wslots = wslots;
  t.owner = owner;
  t.S = S;
  t.rep_end = rep_end;
  if (rep_end != nullptr)
    zk::front_pieces_k<true><<<zk::fg_blocks(S), zk::FG_T, 0, st>>>(
        t, p_stream, p_src, p_len);
  else
    zk::front_pieces_k<false><<<zk::fg_blocks(S), zk::FG_T, 0, st>>>(
        t, p_stream, p_src, p_len);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_front_tx_pieces(const int64_t* rep_off, const int32_t* wslots,
                       const int64_t* const* slot_off, const int32_t* err,
                       const int64_t* caps, int64_t S, int64_t* owner,
                       int32_t* p_stream, int64_t* p_src, int64_t* p_len,
                       int64_t* stats, hipStream_t st) {
  return zk_front_tx_pieces_end(rep_off, nullptr, wslots, slot_off, err, caps,
                                S, owner, p_stream, p_src, p_len, stats, st);
}

}  // extern "C"
