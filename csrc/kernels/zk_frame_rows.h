// K1's (body offset, length) rows from the per-tile frame-start lists that
// fs_tile / fs_link settled (zk_frame_tile.h, frame_link.hip) — the one
// implementation, used by fs_rows (frame_scan.hip: a wave per tile, the plain
// scan's third launch) and by the
// consumers of a rows-deferred scan (decode_replies_k and tree_serve_k's
// TILES instances: a workgroup per block of 256 frames), which then need no
// fs_rows launch and no read-back of the rows it would have written.
//
// Row i of the table lies in the largest tile t <= *lastk with rowbase(t) =
// bsum[t / 64] + base[t] <= i; it is the tile's frame k = i - rowbase(t).
// Its start is pre[k] (k < np) or list[js + k - np], its end the next
// frame's start, or rec_exit[t] for the tile's last frame: no stream byte is
// read.  A STALE tile (fs_link's chase looked its exact entry, exit and
// count up; the recorded starts belong to the old entry) is walked from
// rec_entry[t] through a staged copy of its bytes.
#pragma once
#include "zk_common.h"
#include "zk_stage_span.h"

namespace zk {

constexpr int FT_S = 4096;                 // tile bytes
constexpr int FT_LMAX = FT_S / 4;          // most frame starts a tile holds
constexpr int FT_STAGE = FT_S + 16;        // staged bytes (+ length overhang)
// Count blocks: frame counts scanned per FK_T tiles (one wave's worth)
constexpr int FK_T = 64;
// fs_link's grid words (see fl_check's caller)
constexpr int FL_NB = 2;                   // broken links the check saw
constexpr int FL_GW = FL_NB + 1;
// The workspace's words after the X flags (uint64, lbw + 2 * tiles): [0..3]
// stats, [4..5] the check's minima, [6] the last live tile, [7] this scan's
// tiles without a speculated entry (fs_tile counts; cleared with the rows),
// [8, 8 + FL_GW) fs_link's grid words, [16, 32) its barrier words (the big
// repair, see fs_link)
constexpr int LW_MINS = 4, LW_LAST = 6, LW_NOSPEC = 7, LW_GRID = 8;
constexpr int LW_BIG = 16;
constexpr int LW_END = 32;
static_assert(LW_GRID + FL_GW <= LW_BIG, "grid words");
// frames a consumer workgroup takes (decode.hip DEC_T, zk_tree.h TR_T)
constexpr int FR_T = 256;
// tiles of a consumer's row-base window: 256 rows of a GET stream lie in 3
// request or 12 reply tiles, so one wave's worth of gathers covers them;
// rows of frames longer than a tile take more passes
constexpr int FR_W = 64;

// The scanned length: a producer's device-side byte count clamped to the
// buffer capacity (null: the capacity itself, a host-known length).
ZK_DEV int64_t stream_len(const int64_t* n_dev, int64_t n_cap) {
  if (n_dev == nullptr) return n_cap;
  const int64_t v = *n_dev;
  return v < 0 ? 0 : (v < n_cap ? v : n_cap);
}

// Big-endian i32 at byte p of an LDS image (two aligned dwords + alignbyte).
ZK_DEV int32_t lds_be32(const uint8_t* sb, int32_t p) {
  const int32_t a = p & ~3;
  const uint32_t lo = *(const uint32_t*)(sb + a);
  const uint32_t hi = *(const uint32_t*)(sb + a + 4);
  return (int32_t)bswap32(__builtin_amdgcn_alignbyte(hi, lo, p & 3));
}

// per-tile record: meta = cnt | np << 11 | (js + 1) << 22 | term << 33 |
// bad << 34 (zk_frame_scan.h FcWalk)
ZK_DEV int32_t m_cnt(int64_t m) { return (int32_t)(m & 0x7FF); }
ZK_DEV int32_t m_np(int64_t m) { return (int32_t)((m >> 11) & 0x7FF); }
ZK_DEV int32_t m_js(int64_t m) { return (int32_t)((m >> 22) & 0x7FF) - 1; }
ZK_DEV bool m_term(int64_t m) { return (m >> 33) & 1; }
ZK_DEV bool m_bad(int64_t m) { return (m >> 34) & 1; }
// a tile whose exact entry, exit and frame count fs_link's chase looked up:
// its recorded frame starts are still the old entry's, so its rows are walked
constexpr int64_t M_STALE = (int64_t)1 << 35;
ZK_DEV bool m_stale(int64_t m) { return (m >> 35) & 1; }

// Stage [wb, wb + WIN) (zero past n) into the wave's window: all WIN/1024
// 16-byte loads of a lane issued before the first LDS write.
template <int WIN>
ZK_DEV void fc_stage(const uint8_t* __restrict__ buf, int64_t n, int64_t wb,
                     uint8_t* win, int lane) {
  constexpr int PER = WIN / 1024;
  uint4 v[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int64_t g = wb + 16 * (lane + 64 * j);
    v[j] = make_uint4(0, 0, 0, 0);
    if (g + 16 <= n) {
      __builtin_memcpy(&v[j], buf + g, 16);
    } else if (g < n) {
      uint8_t* b = (uint8_t*)&v[j];
      for (int k = 0; k < 16; ++k) b[k] = g + k < n ? buf[g + k] : 0;
    }
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) *(uint4*)(win + 16 * (lane + 64 * j)) = v[j];
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// fc_stage<FT_S> one 16-byte load a lane at a time: a quarter of the
// registers, for the consumers' stale-tile walk (rare there, and the
// registers of a path never taken would cost every workgroup occupancy).
ZK_DEV void fr_stage_lean(const uint8_t* __restrict__ buf, int64_t n,
                          int64_t wb, uint8_t* win, int lane) {
#pragma unroll 1
  for (int j = 0; j < FT_S / 1024; ++j) {
    const int64_t g = wb + 16 * (lane + 64 * j);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (g + 16 <= n) {
      __builtin_memcpy(&v, buf + g, 16);
    } else if (g < n) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll 1
      for (int k = 0; k < 16; ++k)
        if (g + k < n) w[k >> 2] |= (uint32_t)buf[g + k] << (8 * (k & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4*)(win + 16 * (lane + 64 * j)) = v;
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// N dwords in memory order from byte p of an LDS image (N + 1 aligned
// dwords + alignbyte; reads up to 4 bytes past p + 4 N).
template <int N>
ZK_DEV void lds_words(const uint8_t* sb, int32_t p, uint32_t (&w)[N]) {
  const uint32_t* a = (const uint32_t*)(sb + (p & ~3));
  uint32_t r[N + 1];
#pragma unroll
  for (int k = 0; k <= N; ++k) r[k] = a[k];
#pragma unroll
  for (int k = 0; k < N; ++k)
    w[k] = __builtin_amdgcn_alignbyte(r[k + 1], r[k], p & 3);
}

ZK_DEV int64_t wave_uniform(int64_t x) {     // (x is the same in every lane)
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
  const uint32_t hi =
      __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---- staging a wave's frames in LDS ----------------------------------------
//
// The lanes of a wave that hold consecutive rows (fo, fl), as fr_row hands
// them out, own one contiguous span of the stream: from the first such
// lane's fo to the last one's fo + fl.  fr_span_load + fr_span_store copy it
// into the wave's own LDS image with 16-byte-per-lane coalesced loads
// (zk_stage_span.h: the aligned chunks, the clipped head and tail; no byte
// outside buf[0, n) is read, whatever buf's alignment), and hand each lane
// the image offset of its body.  In two halves, so that a consumer can have
// the loads of several spans in flight (a group of lanes each, one image
// reused) before it waits for the first.
//
// IMG, the consumer's compile-time budget: the image's chunk bytes (a lane
// holds IMG / 1024 chunks).  ONE decision per span, the same in every lane of
// the wave: it is staged when some lane holds a row, every row lies inside
// [s, e), the span lies inside the stream, and head + span fits IMG (a span
// of IMG - 15 bytes always does).  Otherwise nothing is read or written and
// the lanes read their frames from global memory as before.  Wave-private:
// no workgroup barrier.
template <int IMG>
constexpr int fr_image_bytes() { return IMG + 16; }   // + lds_words' overhang

template <int IMG>
struct FrSpan {
  static_assert(IMG % 1024 == 0, "whole chunks a lane");
  static constexpr int PER = IMG / 1024;
  StageSpan sp;
  int64_t s;
  bool ok;
  uint4 v[PER];
};

// The decision, and (span inside the stream's aligned chunks: the common
// case) every load of the lane issued.  mine: this lane holds a row of the
// span.
template <int IMG>
ZK_DEV void fr_span_load(const uint8_t* __restrict__ buf, int64_t n, bool mine,
                         int64_t fo, int32_t fl, int lane, FrSpan<IMG>& F) {
  F.ok = false;
  const uint64_t m = __ballot(mine);
  if (m == 0) return;
  const int first = (int)__builtin_ctzll(m);
  const int last = 63 - (int)__builtin_clzll(m);
  const int64_t s = wave_uniform(__shfl(fo, first, 64));
  const int64_t e = wave_uniform(__shfl(fo + (fl > 0 ? fl : 0), last, 64));
  if (!span_fits(s, e, n, IMG)) return;
  const bool in = !mine || (fl >= 0 && fo >= s && fo + fl <= e);
  if (__ballot(!in) != 0) return;
  F.sp = span_make((uint64_t)(uintptr_t)buf, s, e, n);
  F.s = s;
  if (!span_image_fits(F.sp, IMG)) return;
  F.ok = true;
  if (F.sp.clipped) return;
#pragma unroll
  for (int j = 0; j < FrSpan<IMG>::PER; ++j) {
    const int32_t c = lane + 64 * j;
    F.v[j] = make_uint4(0, 0, 0, 0);
    if (c < F.sp.nchunks)
      __builtin_memcpy(&F.v[j], buf + span_chunk_off(F.sp, c), 16);
  }
}

// The image written (img: 16-byte aligned, fr_image_bytes<IMG>()) and
// visible to the wave; rel = the image offset of this lane's body.  False: the
// span is not staged.
template <int IMG>
ZK_DEV bool fr_span_store(const uint8_t* __restrict__ buf, int64_t n,
                          const FrSpan<IMG>& F, uint8_t* img, int lane,
                          int64_t fo, int32_t& rel) {
  if (!F.ok) return false;
  if (!F.sp.clipped) {
#pragma unroll
    for (int j = 0; j < FrSpan<IMG>::PER; ++j) {
      const int32_t c = lane + 64 * j;
      if (c < F.sp.nchunks) *(uint4*)(img + 16 * c) = F.v[j];
    }
  } else {
#pragma unroll 1
    for (int32_t c = lane; c < F.sp.nchunks; c += 64) {
      uint32_t w[4];
      span_load_chunk(buf, n, F.sp, c, w);
      *(uint4*)(img + 16 * c) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  rel = F.sp.head + (int32_t)(fo - F.s);
  return true;
}

// Frame k (< cnt) of tile t from its recorded starts: start p and end q
// (stream offsets of the length word and of the byte after the body).  A
// frame ends where the next one of the chain starts, the tile's last at the
// tile's exit x (the next tile's first frame, or the stop offset of a
// terminal tile).
ZK_DEV void fr_bounds(const uint16_t* __restrict__ list,
                      const uint16_t* __restrict__ pre, int64_t t, int64_t m,
                      int64_t x, int32_t k, int64_t& p, int64_t& q) {
  const int32_t cnt = m_cnt(m), np = m_np(m), js = m_js(m);
  const int64_t ts = t * FT_S;
  const uint16_t* P = pre + t * FT_LMAX;
  const uint16_t* R = list + t * FT_LMAX + (js < 0 ? 0 : js);
  p = ts + (k < np ? P[k] : R[k - np]);
  const int32_t k1 = k + 1;
  q = k1 < cnt ? ts + (k1 < np ? P[k1] : R[k1 - np]) : x;
}

// The rows of a stale tile t (cnt frames from tile-relative entry c, exit
// x), by ONE wave: the tile is staged into sb (FT_STAGE bytes) and walked;
// the walk keeps 64 starts in the lanes (lane k & 63 holds start k) and
// emits their rows every 64 frames: emit(k, start, end) in every lane that
// holds one.  LEAN: staged with fr_stage_lean.
template <bool LEAN, typename Emit>
ZK_DEV void fr_walk_stale(const uint8_t* __restrict__ buf, int64_t n,
                          int64_t t, int32_t c, int32_t cnt, int64_t x,
                          uint8_t* sb, int lane, Emit emit) {
  const int64_t ts = t * FT_S;
  if (LEAN) fr_stage_lean(buf, n, ts, sb, lane);
  else fc_stage<FT_S>(buf, n, ts, sb, lane);
  if (lane == 0) {
    uint8_t* pb = sb + FT_S;
#pragma unroll 1
    for (int k = 0; k < 16; ++k)
      pb[k] = ts + FT_S + k < n ? buf[ts + FT_S + k] : 0;
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int32_t ent = 0;
  for (int32_t k = 0; k < cnt; ++k) {
    ent = lane == (k & 63) ? c : ent;
    const int32_t len = __builtin_amdgcn_readfirstlane(lds_be32(sb, c));
    c += 4 + len;
    if ((k & 63) == 63 || k == cnt - 1) {
      const int32_t last = k & 63;
      const int32_t nxt = __shfl_down(ent, 1, 64);
      if (lane <= last) {
        const int64_t p = ts + ent;
        const int64_t q = lane < last ? ts + nxt
                                      : (k == cnt - 1 ? x : ts + c);
        emit((k & ~63) + lane, p, q);
      }
    }
  }
}

// ---- the consumers' side ---------------------------------------------------

// A consumer workgroup's LDS: the row bases of a window of tiles (relative
// to the workgroup's first row), the rows a stale tile's walk found, and
// ONE tile stage for those walks (wave 0's; a stage per wave would cost the
// consumers occupancy for a path that is rare).
struct FrLds {
  __attribute__((aligned(16))) uint8_t stage[FT_STAGE];
  int64_t off[FR_T];
  int32_t len[FR_T];
  int32_t rb[FR_W];
  unsigned long long pick;
};

ZK_DEV int64_t fr_rowbase(const ZkFrameTiles& T, int64_t t) {
  return T.bsum[t / FK_T] + T.base[t];
}

// The (body offset, length) row of this thread's frame i = FR_T * blk +
// threadIdx.x, exactly as fs_rows writes it, for i < nrows (= min(frames
// found, table capacity)); false past that.  Every thread of the workgroup
// calls it (FR_T threads, barriers inside).
ZK_DEV bool fr_row(const ZkFrameTiles& T, uint32_t blk, int64_t nrows,
                   FrLds& S, int64_t& foff, int32_t& flen) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t i0 = (int64_t)blk * FR_T;
  if (i0 >= nrows) return false;                     // (workgroup-uniform)
  const bool act = i0 + tid < nrows;
  const int64_t n = stream_len(T.n_dev, T.n_cap);
  const int64_t lastk = *T.lastk;
  // LOCATE: the count block of row i0 from fs_link's index, then the first
  // tile with one wave-wide look at the block's 64 row bases
  int64_t w0;
  {
    const int64_t b = T.fblk[blk];
    const int64_t t = b * FK_T + lane;
    const bool le = t <= lastk && fr_rowbase(T, t) <= i0;
    const uint64_t m = __ballot(le);
    w0 = b * FK_T + (m ? 63 - (int64_t)__builtin_clzll(m) : 0);
  }
  // WINDOW LOOP: the row bases of FR_W tiles from w0 on (wave 0 loads them); a thread's tile is
  // the largest with rowbase <= its row (tiles without a frame, under a
  // frame longer than a tile, share the next one's base and are skipped).
  // A thread whose row may lie past the window waits for the next, which
  // starts at this one's last tile.
  int64_t t = -1;
  int32_t k = 0;
  bool placed = !act;
  for (;;) {
    if (tid < FR_W) {
      const int64_t tw = w0 + tid;
      int32_t r = 0x7FFFFFFF;
      if (tw <= lastk) {
        const int64_t d = fr_rowbase(T, tw) - i0;
        r = d > FR_T ? FR_T : (int32_t)d;
      }
      S.rb[tid] = r;
    }
    __syncthreads();
    if (!placed) {
      int lo = 0;                    // rb[0] <= 0 <= tid: the answer exists
#pragma unroll
      for (int s = FR_W / 2; s >= 1; s >>= 1)
        if (S.rb[lo + s] <= tid) lo += s;
      if (lo < FR_W - 1 || w0 + FR_W - 1 >= lastk) {
        t = w0 + lo;
        k = tid - S.rb[lo];
        placed = true;
      }
    }
    if (!__syncthreads_or(!placed)) break;
    w0 += FR_W - 1;
  }
  // FRAME BOUNDS from the tile's recorded starts
  int64_t m = 0, x = 0;
  bool stale = false;
  if (act) {
    m = T.rec_meta[t];
    x = T.rec_exit[t];
    stale = m_stale(m);
    foff = 0;
    flen = 0;
    // (k < cnt by the row bases; a record that broke that must not send
    // the reads below past the tile's lists)
    if (!stale && (uint32_t)k < (uint32_t)m_cnt(m)) {
      int64_t p, q;
      fr_bounds(T.list, T.pre, t, m, x, k, p, q);
      foff = p + 4;
      flen = (int32_t)(q - p - 4);
    }
  }
  // STALE TILES of the workgroup's range, one after the other (the smallest
  // first): wave 0 walks the tile, the threads whose rows are its frames
  // take them from LDS
  if (__syncthreads_or(stale)) {
    for (;;) {
      if (tid == 0) S.pick = ~0ull;
      __syncthreads();
      if (stale) atomicMin(&S.pick, (unsigned long long)t);
      __syncthreads();
      const unsigned long long pk = S.pick;
      if (pk == ~0ull) break;
      const int64_t tt = (int64_t)pk;
      if (stale && t == tt) {
        S.off[tid] = 0;
        S.len[tid] = 0;
      }
      __syncthreads();
      if (tid < 64) {
        const int64_t mt = T.rec_meta[tt];
        const int64_t rel = fr_rowbase(T, tt) - i0;    // (may be negative)
        const int32_t c = __builtin_amdgcn_readfirstlane(
            (int32_t)(T.rec_entry[tt] - tt * FT_S));
        fr_walk_stale<true>(T.buf, n, tt, c, m_cnt(mt), T.rec_exit[tt], S.stage,
                      lane, [&](int32_t kk, int64_t p, int64_t q) {
                        const int64_t r = rel + kk;
                        if (r >= 0 && r < FR_T) {
                          S.off[r] = p + 4;
                          S.len[r] = (int32_t)(q - p - 4);
                        }
                      });
      }
      __syncthreads();
      if (stale && t == tt) {
        foff = S.off[tid];
        flen = S.len[tid];
        stale = false;
      }
      __syncthreads();
    }
  }
  return act;
}

// What fs_rows does for the NEXT scan of the workspace, by a consumer's
// grid: the candidate flags of every tile below the stream length cleared
// (a strided share a workgroup; tiles past *lastk included, which no row
// maps to), and fs_link's minima, no-speculation count, broken-link count
// and barrier words.  zk_frame_scan may then run with clean = 1.
ZK_DEV void fr_housekeep(const ZkFrameTiles& T) {
  const int64_t n = stream_len(T.n_dev, T.n_cap);
  const int64_t ntiles = (n + FT_S - 1) / FT_S;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ntiles;
       t += step) {
    T.lbw[2 * t] = 0;
    T.lbw[2 * t + 1] = 0;
  }
  if (blockIdx.x == 0) {
    uint64_t* tail = T.lbw + 2 * T.tiles;
    const int tid = threadIdx.x;
    if (tid == 0) {
      tail[LW_MINS] = 0;
      tail[LW_MINS + 1] = 0;
      tail[LW_NOSPEC] = 0;
      tail[LW_GRID + FL_NB] = 0;
    }
    if (tid < LW_END - LW_BIG) tail[LW_BIG + tid] = 0;
  }
}

}  // namespace zk
