// K1's tile pass: everything fs_tile is made of (the kernel is a template;
// frame_tile.hip, frame_group256.hip and frame_group512.hip instantiate and
// launch it).  The design note: zk_frame_scan.h.
#pragma once
#include "zk_frame_scan.h"
#include "zk_run_span.h"

namespace zk {

constexpr int FT_BITS = FT_S / 32;         // uint32 words per position map
constexpr int FT_XW = 2048 / 32;           // exit candidates: the next tile's
                                           // window positions (W <= 2048)

// Record frame start c as entry m of a list in global memory: lane m & 63
// keeps it in `ent`, every 64 entries leave in one coalesced store.
ZK_DEV void ft_record(uint16_t* L, int32_t& m, uint32_t& ent, int32_t c,
                      int lane) {
  ent = lane == (m & 63) ? (uint32_t)c : ent;
  ++m;
  if ((m & 63) == 0) L[m - 64 + lane] = (uint16_t)ent;
}

// The survivor's frame starts below tile position c: the popcount of its
// bits under c (two map words a lane).
ZK_DEV int32_t ft_starts_below(const uint32_t* sbits, int32_t c, int lane) {
  static_assert(FT_BITS == 2 * 64, "two map words per lane");
  const int32_t cw = c >> 5;
  int32_t below = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int32_t wi = lane + 64 * h;
    const uint32_t wd = sbits[wi];
    below += wi < cw ? __popc(wd)
                     : (wi == cw ? __popc(wd & ((1u << (c & 31)) - 1u)) : 0);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) below += __shfl_xor(below, d, 64);
  return below;
}

// The chain from tile-relative candidate entry e, walked in LDS (wave-
// uniform): does it survive this tile, and where does it leave it?
// Returns the absolute exit (>= the tile end) when it leaves the tile, or
// meets the survivor's path and the survivor leaves (its exit `send`),
// packed with the number of frames the chain starts in this tile
// (cx_exit / cx_cnt); FC_DEAD when it hits a bad length or meets a
// survivor that ends on one; FC_LIVE when it survives without a known exit
// (it reaches the stream end, or meets a survivor that ends there).
// fs_link's chase takes these as the tile's entry -> (exit, count) map.
// (fs_tile answers most candidates from its chain map; this exact walk is
// the fallback for chains the map leaves open.)
ZK_DEV int64_t ft_cand(const uint8_t* sb, const uint32_t* sbits, int32_t e,
                       int32_t nrel, int32_t maxp, int64_t send, int64_t n,
                       int64_t ts, int32_t m, int lane) {
  int32_t c = e;
  int32_t hops = 0;
  for (;;) {
    if (c >= FT_S) return (ts + c) | ((int64_t)hops << CX_SHIFT);
    if (ts + c >= n) return FC_LIVE;
    // the survivor-map word and the length word, read together (the map
    // is all zero without a survivor)
    const uint32_t smw = sbits[c >> 5];
    const int32_t lraw = lds_be32(sb, c);
    if ((smw >> (c & 31)) & 1u) {
      if (send & TERM) return (send & TBAD) ? FC_DEAD : FC_LIVE;
      // joined: the survivor's frames from its start at c on (their index
      // is the number of survivor starts below c; two map words a lane)
      const int32_t below = ft_starts_below(sbits, c, lane);
      return send | ((int64_t)(hops + m - below) << CX_SHIFT);
    }
    if (c + 4 > nrel) return FC_LIVE;
    const int32_t len = __builtin_amdgcn_readfirstlane(lraw);
    if ((uint32_t)len > (uint32_t)maxp) return FC_DEAD;
    const int32_t nx = c + 4 + len;
    if (nx > nrel) return FC_LIVE;
    ++hops;
    c = nx;
  }
}

// ---- fs_tile: the tile's chain map, by pointer jumping ---------------------
//
// Every position p of the tile whose length word reads as a plausible frame
// body (minb <= len <= W - 4, the window covering the stream's frames;
// < FT_LIMIT in long-frame mode; in the entry window also any length up to
// maxp) is a NODE.  A node's successor is the next frame start, p + 4 + len:
// another node, or a ROOT where the chain ends inside the tile's view —
//   EXIT   the chain leaves the tile (val = its last frame's start: the exit
//          is that frame's end, read from the staged bytes);
//   END    the stream ends exactly at the last frame's end (val = its start);
//   PART   a frame (val) is cut by the stream end (its header or body);
//   BAD    a frame (val) has a length < 0 or > maxp (BAD_LENGTH);
//   SHORT  a frame (val) has a legal length below minb: the map does not
//          follow it (an exact serial walk does, when the chain matters).
// Pointer jumping (each round: node -> successor's successor, counts
// added) takes every node to its root in log2(frames per tile) rounds, all
// lanes busy: ~5 rounds on 192-byte frames, ~7 on 42-byte ones, where the
// round-3 kernel walked ~20 / ~90 dependent LDS hops on one lane after a
// merging frontier.  Lane l holds nodes l, l + 64, ... in registers (their
// positions and words), and every phase issues all of its LDS reads before
// it waits.  The map then answers, in O(1) each, what the tile chain logic
// needs: the exits of the window entries (the next tile's candidate
// entries), the survival / exit / frame count of the tile before's
// candidates (fs_link's candidate exit map), and the frame starts of the
// chosen entry's chain (slot index = count - the node's count to the root;
// a side branch landing on the chain is caught by the successor check and
// sent to the serial walk).  What fs_link / fs_rows read is
// unchanged: entry, exit, count, frame-start lists and candidate exits.
constexpr int FT_NMAX = 512;               // nodes a tile's map holds (GET
                                           // streams: 240-340; more: the
                                           // serial walks)
constexpr int FT_SLOTS = 352;              // chain slots (frames >= 12 bytes)
constexpr int32_t FT_LIMIT = FT_S;         // node lengths below this
enum : uint32_t {
  RK_NODE = 0, RK_EXIT = 1, RK_END = 2, RK_PART = 3, RK_BAD = 4, RK_SHORT = 5
};
// node word: kind (3 bits) | val (13 bits: successor node or a position) |
// frame starts from the node to the root (16 bits)
ZK_DEV uint32_t rk(uint32_t kind, uint32_t val, uint32_t cnt) {
  return kind << 29 | val << 16 | cnt;
}
ZK_DEV uint32_t rk_kind(uint32_t w) { return w >> 29; }
ZK_DEV uint32_t rk_val(uint32_t w) { return (w >> 16) & 0x1FFF; }
ZK_DEV uint32_t rk_cnt(uint32_t w) { return w & 0xFFFF; }

// LDS layout per wave (7.6 KiB: 20 waves a CU): staged tile | node masks
// of the 64 position blocks | nodes before each block | node words | R:
// node positions while the map is built, then the chain slots (or the
// serial walks' survivor bits) and the exit candidate bits
constexpr int FT_SLOT_B = 704;             // >= FT_SLOTS * 2, >= FT_BITS * 4
constexpr int FT_O_BLK = FT_STAGE;         // uint64 [64]
constexpr int FT_O_BASE = FT_O_BLK + 64 * 8;   // uint16 [64]
constexpr int FT_O_PK = FT_O_BASE + 64 * 2;
constexpr int FT_O_R = FT_O_PK + FT_NMAX * 4;
constexpr int FT_R_B = FT_NMAX * 2 > FT_SLOT_B + FT_XW * 4
                           ? FT_NMAX * 2 : FT_SLOT_B + FT_XW * 4;
constexpr int FT_O_XB = FT_O_R + FT_SLOT_B;
constexpr int FT_LDS = FT_O_R + FT_R_B;
static_assert(FT_SLOT_B >= FT_SLOTS * 2 && FT_SLOT_B >= FT_BITS * 4, "slots");
static_assert(FT_STAGE % 16 == 0 && FT_LDS % 16 == 0, "LDS alignment");

// Big-endian i32 at byte p from the two aligned dwords around it.
ZK_DEV int32_t be32_of(uint32_t lo, uint32_t hi, int32_t p) {
  return (int32_t)bswap32(__builtin_amdgcn_alignbyte(hi, lo, p & 3));
}

// The node map of a tile: a mask of nodes per 64-position block and the
// nodes before each block (node indices follow positions).
struct FtBlk {
  const uint64_t* mask;
  const uint16_t* base;
};

// Is tile position q (< FT_S) a node; its index if so.
ZK_DEV bool ft_node(const FtBlk& blk, int32_t q, int32_t& idx) {
  const uint64_t m = blk.mask[q >> 6];
  const int32_t b = blk.base[q >> 6];
  const uint64_t bit = 1ull << (q & 63);
  idx = b + __popcll(m & (bit - 1));
  return (m & bit) != 0;
}

// The root word of a chain continuing at NON-node position q (< FT_S) whose
// length word reads len, after `before` frame starts.
ZK_DEV uint32_t ft_classify(int32_t q, int32_t len, int32_t nrel,
                            int32_t maxp, int32_t minb, uint32_t before) {
  if (q + 4 > nrel) return rk(RK_PART, q, before);
  if ((uint32_t)len > (uint32_t)maxp) return rk(RK_BAD, q, before);
  const int32_t nx = q + 4 + len;
  if (nx > nrel) return rk(RK_PART, q, before);
  if (len < minb) return rk(RK_SHORT, q, before);
  // a legal length >= FT_LIMIT (not a node): the frame leaves the tile
  if (nx >= FT_S) return rk(RK_EXIT, q, before + 1);
  return nx == nrel ? rk(RK_END, q, before + 1) : rk(RK_SHORT, q, before);
}

// Root word of the chain entering at tile position e (wave-uniform; e <
// nrel, the map built).
ZK_DEV uint32_t ft_root_at(const uint8_t* sb, const FtBlk& blk,
                           const uint32_t* pk, int32_t e, int32_t nrel,
                           int32_t maxp, int32_t minb) {
  int32_t j;
  if (ft_node(blk, e, j)) return pk[j];
  return ft_classify(e, lds_be32(sb, e), nrel, maxp, minb, 0);
}

// End of the frame starting at tile position p (its length word staged).
ZK_DEV int32_t ft_next(const uint8_t* sb, int32_t p) {
  return p + 4 + lds_be32(sb, p);
}

// The candidate-exit value (ft_cand's) of a chain with root word w.
ZK_DEV int64_t ft_cx(const uint8_t* sb, uint32_t w, int64_t ts) {
  switch (rk_kind(w)) {
    case RK_EXIT:
      return (ts + ft_next(sb, (int32_t)rk_val(w))) |
             ((int64_t)rk_cnt(w) << CX_SHIFT);
    case RK_BAD: return FC_DEAD;
    default: return FC_LIVE;                 // END / PART
  }
}

// The survivor end code (sx) of a chain with root word w.
ZK_DEV int64_t ft_send(const uint8_t* sb, uint32_t w, int64_t ts) {
  const int32_t v = (int32_t)rk_val(w);
  switch (rk_kind(w)) {
    case RK_EXIT: return ts + ft_next(sb, v);
    case RK_END: return TERM | (ts + ft_next(sb, v));
    case RK_BAD: return TERM | TBAD | (ts + v);
    default: return TERM | (ts + v);         // PART
  }
}

// This lane's nodes i = lane + 64 k: positions (-1: none) and words.
template <int NK>
struct FtNodes {
  int32_t p[NK];
  uint32_t w[NK];
};

// Successors of this lane's nodes, then pointer jumping until every node's
// word is its root's (kind, val) with the frame count from it.  Returns the
// jumping rounds.
template <int NK>
ZK_DEV int ft_build(FtNodes<NK>& me, const uint8_t* sb, const FtBlk& blk,
                    uint32_t* pk, const uint16_t* pos, int32_t N,
                    int32_t nrel, int32_t maxp, int32_t minb, int lane) {
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int32_t i = lane + 64 * k;
    const int32_t p = pos[i < N ? i : 0];
    me.p[k] = i < N ? p : -1;
  }
  uint32_t a[NK], b[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int32_t q = me.p[k] < 0 ? 0 : me.p[k] & ~3;
    a[k] = *(const uint32_t*)(sb + q);
    b[k] = *(const uint32_t*)(sb + q + 4);
  }
  int32_t nx[NK];
  uint64_t bm[NK];
  uint32_t bb[NK], c[NK], d[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int32_t p = me.p[k] < 0 ? 0 : me.p[k];
    nx[k] = p + 4 + be32_of(a[k], b[k], p);
    const int32_t q = nx[k] < FT_S ? nx[k] : 0;
    bm[k] = blk.mask[q >> 6];
    bb[k] = blk.base[q >> 6];
    c[k] = *(const uint32_t*)(sb + (q & ~3));
    d[k] = *(const uint32_t*)(sb + (q & ~3) + 4);
  }
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int32_t p = me.p[k];
    const int32_t q = nx[k];
    uint32_t r;
    if (q > nrel) {
      r = rk(RK_PART, p, 0);
    } else if (q >= FT_S) {
      r = rk(RK_EXIT, p, 1);
    } else if (q == nrel) {
      r = rk(RK_END, p, 1);
    } else {
      const uint64_t bit = 1ull << (q & 63);
      if (bm[k] & bit)
        r = rk(RK_NODE, bb[k] + __popcll(bm[k] & (bit - 1)), 1);
      else
        r = ft_classify(q, be32_of(c[k], d[k], q), nrel, maxp, minb, 1);
    }
    me.w[k] = r;
    if (p >= 0) pk[lane + 64 * k] = r;
  }
  __builtin_amdgcn_wave_barrier();
  int rounds = 0;
  for (;;) {
    uint32_t q[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const bool go = me.p[k] >= 0 && rk_kind(me.w[k]) == RK_NODE;
      q[k] = pk[go ? rk_val(me.w[k]) : 0];
    }
    bool more = false;
    uint32_t nw[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      nw[k] = me.w[k];
      if (me.p[k] >= 0 && rk_kind(me.w[k]) == RK_NODE) {
        nw[k] = (q[k] & 0xFFFF0000u) | (rk_cnt(me.w[k]) + rk_cnt(q[k]));
        more |= rk_kind(q[k]) == RK_NODE;
      }
    }
    // every read of the round is issued before its first write (the
    // wave's LDS operations complete in order)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if (nw[k] != me.w[k]) pk[lane + 64 * k] = nw[k];
      me.w[k] = nw[k];
    }
    __builtin_amdgcn_wave_barrier();
    ++rounds;
    if (!__ballot(more)) break;
  }
  return rounds;
}

// The window entries' exits into xbits (this tile's candidate entries of
// the next one) and the preferred chain: the window entry with the longest
// chain, else (LONG) the first node whose chain leaves the tile.  Returns
// its position (-1: none) and its exit past the tile end in `sx`.
template <int W, bool LONG, int NK>
ZK_DEV int32_t ft_cands(const FtNodes<NK>& me, const uint8_t* sb,
                        uint32_t* xbits, int32_t& sx) {
  uint32_t a[NK], b[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const bool ex = rk_kind(me.w[k]) == RK_EXIT && me.p[k] >= 0 &&
                    (LONG || me.p[k] < W);
    const int32_t v = ex ? (int32_t)rk_val(me.w[k]) : 0;
    a[k] = *(const uint32_t*)(sb + (v & ~3));
    b[k] = *(const uint32_t*)(sb + (v & ~3) + 4);
  }
  // keys: (count, -position) above the exit, so the max carries its exit
  uint64_t best = 0, first = 0;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int32_t p = me.p[k];
    if (p < 0 || rk_kind(me.w[k]) != RK_EXIT || (!LONG && p >= W)) continue;
    const int32_t v = (int32_t)rk_val(me.w[k]);
    const uint32_t x = (uint32_t)(v + 4 + be32_of(a[k], b[k], v) - FT_S);
    if (p < W) {
      if (x < (uint32_t)W)
        __hip_atomic_fetch_or(&xbits[x >> 5], 1u << (x & 31),
                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      const uint64_t key = (uint64_t)(rk_cnt(me.w[k]) << 16 |
                                      (uint32_t)(0xFFFF - p)) << 32 | x;
      best = best > key ? best : key;
    } else if (LONG) {
      const uint64_t key = (uint64_t)(0xFFFF - p) << 32 | x;
      first = first > key ? first : key;
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((long long)best, s, 64);
    best = best > o ? best : o;
    if (LONG) {
      const uint64_t f = (uint64_t)__shfl_xor((long long)first, s, 64);
      first = first > f ? first : f;
    }
  }
  const uint64_t k = best ? best : (LONG ? first : 0);
  if (!k) return -1;
  sx = (int32_t)(uint32_t)k;
  return 0xFFFF - (int32_t)((k >> 32) & 0xFFFF);
}

// ft_cands for a tile without a map (more than FT_NMAX nodes: payloads of
// small big-endian words, each a plausible length).  The window's first
// 128 nodes are walked, one chain per lane and round, all lanes at once
// (per-lane LDS hops); their exits and the preferred chain are chosen as
// ft_cands chooses them.  Without this the tile published no candidate,
// the next one had no speculated entry, and a run of such tiles became a
// serial repair.
template <int W>
ZK_DEV int32_t ft_cands_walk(const uint8_t* sb, const FtBlk& blk,
                             uint32_t* xbits, int32_t nrel, int32_t maxp,
                             int32_t& sx, int lane) {
  uint64_t best = 0;
  for (int r = 0; r < 2; ++r) {
    // this lane's window node: index lane + 64 r in position order
    int32_t want = lane + 64 * r, p = -1;
    for (int b = 0; b < W / 64 && p < 0; ++b) {
      uint64_t m = blk.mask[b];
      const int32_t c = __popcll(m);
      if (want < c) {
        for (int k = 0; k < want; ++k) m &= m - 1;
        p = b * 64 + (int32_t)__builtin_ctzll(m);
      } else {
        want -= c;
      }
    }
    if (!__ballot(p >= 0)) break;
    int32_t c = p, cnt = 0, x = -1;
    bool live = p >= 0;
    while (live) {
      if (c + 4 > nrel) break;
      const int32_t len = lds_be32(sb, c);
      if ((uint32_t)len > (uint32_t)maxp) break;
      const int32_t nx = c + 4 + len;
      if (nx > nrel) break;
      ++cnt;
      if (nx >= FT_S) { x = nx - FT_S; break; }
      c = nx;
    }
    if (x >= 0) {
      if (x < W)
        __hip_atomic_fetch_or(&xbits[x >> 5], 1u << (x & 31),
                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      const uint64_t key = (uint64_t)((uint32_t)cnt << 16 |
                                      (uint32_t)(0xFFFF - p)) << 32 |
                           (uint32_t)x;
      best = best > key ? best : key;
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((long long)best, s, 64);
    best = best > o ? best : o;
  }
  if (!best) return -1;
  sx = (int32_t)(uint32_t)best;
  return 0xFFFF - (int32_t)((best >> 32) & 0xFFFF);
}

// The frame starts of the chain entering at tile position e with root word
// w into the wave's slots (slot k = the k-th start): every node of that
// root with count c <= D at or after e lands in slot D - c; the successor
// check over the slots rejects a side branch sharing the root and count.
// Returns D, or -1 when the chain needs the exact serial walk.
template <int NK>
ZK_DEV int32_t ft_chain(const FtNodes<NK>& me, const uint8_t* sb,
                        const FtBlk& blk, uint16_t* slot, int32_t e,
                        uint32_t w, int lane) {
  const uint32_t kind = rk_kind(w);
  const int32_t D = (int32_t)rk_cnt(w);
  if (kind == RK_SHORT || kind == RK_BAD || D > FT_SLOTS) return -1;
  if (D == 0) return 0;
  const uint32_t root = w >> 16;
  int32_t hits = 0;
  bool on[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int32_t c = (int32_t)rk_cnt(me.w[k]);
    const int32_t p = me.p[k];
    on[k] = p >= e && (me.w[k] >> 16) == root && c >= 1 && c <= D;
    if (on[k]) slot[D - c] = (uint16_t)p;
    hits += __popcll(__ballot(on[k]));
  }
  __builtin_amdgcn_wave_barrier();
  // the chain's nodes: its D frame starts, less the last one when that
  // frame (a long one) is not a node
  int32_t want = D;
  if (lane == 0) {
    slot[0] = (uint16_t)e;
    if (kind == RK_EXIT || kind == RK_END) slot[D - 1] = (uint16_t)rk_val(w);
  }
  if (kind == RK_EXIT || kind == RK_END) {
    int32_t j;
    if (!ft_node(blk, (int32_t)rk_val(w), j)) --want;
  }
  __builtin_amdgcn_wave_barrier();
  // as many hits as chain nodes: no side branch shares the root and a
  // count, every slot holds the chain's start
  if (hits == want) return D;
  // the successor check: every slot's frame ends at the next slot
  auto linked = [&]() {
    bool ok = true;
    for (int32_t k = lane; k < D; k += 64) {
      const int32_t p = slot[k];
      const int32_t nx = ft_next(sb, p);
      if (k + 1 < D) {
        ok &= nx == (int32_t)slot[k + 1];
      } else if (kind == RK_PART) {
        ok &= nx == (int32_t)rk_val(w);
      }
    }
    return __ballot(!ok) == 0;
  };
  if (linked()) return D;
  // Side branches share the root and a count: a length-like word inside a
  // frame that ends where its frame does — a create reply's path length
  // (4 + len past it is the next frame's start: every storm reply frame) —
  // lands on the chain one frame on, and the slot may hold it.  The chain's
  // start is the first of them, so each slot keeps its smallest position
  // (a few rounds: lanes writing one slot at once leave any of their
  // values), and the successor check decides again.  Without it every storm
  // reply tile took the serial walk (24 us of its 77,
  // tools/microbench/k1_bench.py --workload storm).
  for (int it = 0; it < 8; ++it) {
    int32_t cur[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k)
      cur[k] = on[k] ? (int32_t)slot[D - (int32_t)rk_cnt(me.w[k])] : 0;
    bool wr = false;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if (on[k] && me.p[k] < cur[k]) {
        slot[D - (int32_t)rk_cnt(me.w[k])] = (uint16_t)me.p[k];
        wr = true;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (!__ballot(wr)) break;
  }
  return linked() ? D : -1;
}

// ---- staging a tile, walking a chain through it ----------------------------

// Stage the 4 KiB tile at ts in registers (zero past n) / into LDS.
struct FtTileRegs {
  uint4 v[FT_S / 16 / 64];
  uint4 pad;
};
ZK_DEV void ft_load(const uint8_t* __restrict__ buf, int64_t n, int64_t ts,
                    int lane, FtTileRegs& r) {
  constexpr int PER = FT_S / 16 / 64;
  r.pad = make_uint4(0, 0, 0, 0);
  if (ts + FT_STAGE <= n) {
#pragma unroll
    for (int j = 0; j < PER; ++j)
      __builtin_memcpy(&r.v[j], buf + ts + 16 * (lane + 64 * j), 16);
    if (lane == 0) __builtin_memcpy(&r.pad, buf + ts + FT_S, 16);
  } else {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      uint8_t* b = (uint8_t*)&r.v[j];
      const int64_t g = ts + 16 * (lane + 64 * j);
      for (int k = 0; k < 16; ++k) b[k] = g + k < n ? buf[g + k] : 0;
    }
    if (lane == 0) {
      uint8_t* b = (uint8_t*)&r.pad;
      for (int k = 0; k < 16; ++k)
        b[k] = ts + FT_S + k < n ? buf[ts + FT_S + k] : 0;
    }
  }
}
ZK_DEV void ft_store(uint8_t* sb, const FtTileRegs& r, int lane) {
  constexpr int PER = FT_S / 16 / 64;
#pragma unroll
  for (int j = 0; j < PER; ++j) *(uint4*)(sb + 16 * (lane + 64 * j)) = r.v[j];
  if (lane == 0) *(uint4*)(sb + FT_S) = r.pad;
  __builtin_amdgcn_wave_barrier();
}

// The chain from tile-relative c through the staged tile (wave-uniform),
// its frame starts into L; returns the end code (sx) and the count.
// After two frames of one size, a hop reads besides the frame's length
// word (lane 0) the words where the next 63 frames start if they are of
// that size too (lane l: l frames on), so a run of equal frames — every GET
// reply of a 100-byte node is 192 bytes — is taken in one step: the
// leading lanes whose word repeats the length.  One LDS round trip a step
// either way (a group's walked tiles were ~20 dependent hops each, 34 us
// of a 47 us group, tools/microbench/k1_bench.py); streams of varied
// frames keep the one-address hop (a vector address on every hop cost the
// 0-200 B GET stream 3 %) and the records gathered 64 to a store.
// `last` carries the last frame's size across tiles (in: of the frame that
// ends at c, 0 when unknown; out: of the walk's last frame), so a walked tile
// of a run begins with run steps; `run` (out): the walk's last two frames were
// of one size.
ZK_DEV int64_t ft_walk(const uint8_t* sb, int32_t c, int32_t nrel,
                       int32_t maxp32, int64_t ts, uint16_t* L, int32_t& mo,
                       int lane, int32_t& last, bool& run) {
  int32_t m = 0, pb = 0;              // records [pb, m) pending in ent
  uint32_t ent = 0;
  int64_t send;
  // (the walk is wave-uniform: the position and the bounds in SGPRs)
  c = __builtin_amdgcn_readfirstlane(c);
  nrel = __builtin_amdgcn_readfirstlane(nrel);
  last = __builtin_amdgcn_readfirstlane(last);
  run = false;
  const int32_t lim = min((int32_t)FT_S, nrel);
  if (c >= nrel) {
    send = TERM | (ts + c);
  } else {
    int32_t len = 0, nx = 0;
    bool ok = true, fin = false;
    while (!fin) {
      len = __builtin_amdgcn_readfirstlane(lds_be32(sb, c));
      nx = c + 4 + len;
      ok = (uint32_t)len <= (uint32_t)maxp32 && nx <= nrel;
      if (!ok) break;
      ent = lane == (m & 63) ? (uint32_t)c : ent;
      ++m;
      if ((m & 63) == 0) {
        const int32_t q = m - 64 + lane;
        if (q >= pb) L[q] = (uint16_t)ent;
        pb = m;
      }
      if (nx >= lim) {
        run = 4 + len == last;
        last = 4 + len;
        break;
      }
      c = nx;
      if (4 + len != last) {
        last = 4 + len;
        run = false;
        continue;
      }
      run = true;
      // two frames of one size: steps over the run (lane l reads where
      // frame l of it would start); frames 0 .. a-1 lie back to back with
      // that length, and the walk ends after the first reaching the tile's
      // end.  A step that takes none goes back to the hop above.
      const int32_t st = last;
      for (;;) {
        const int64_t s64 = (int64_t)c + (int64_t)lane * st;
        const int32_t sp = s64 < lim ? (int32_t)s64 : lim;
        const int32_t lv = sp < lim ? lds_be32(sb, sp) : -1;
        const bool acc = sp < lim && lv == st - 4 && sp + st <= nrel;
        const uint64_t no = ~__ballot(acc);
        const int32_t a = no ? (int32_t)__builtin_ctzll(no) : 64;
        if (a == 0) break;
        const uint64_t end = __ballot(acc && sp + st >= lim);
        const int32_t f = end ? (int32_t)__builtin_ctzll(end) : 64;
        const int32_t r = min(a, f + 1);
        const int32_t q = (m & ~63) + lane;
        if (q >= pb && q < m) L[q] = (uint16_t)ent;
        if (lane < r) L[m + lane] = (uint16_t)sp;
        m += r;
        pb = m;
        nx = c + r * st;
        len = st - 4;
        if (nx >= lim) {
          fin = true;
          break;
        }
        c = nx;
      }
    }
    if (!ok) {
      const bool bad = (c + 4 <= nrel) && ((len < 0) | (len > maxp32));
      send = TERM | (bad ? TBAD : 0) | (ts + c);
    } else if (nx >= FT_S) {
      send = ts + nx;
    } else {
      send = TERM | (ts + nx);               // the stream ends at nx
    }
  }
  {
    const int32_t q = (m & ~63) + lane;
    if (q >= pb && q < m) L[q] = (uint16_t)ent;
  }
  mo = m;
  return send;
}

// The candidate word of tile t - 1, which is running or done (0: not within
// FT_WAIT_TICKS — no speculation).  Polled with exponential back-off: these
// loads bypass the caches, and thousands of waves polling every few hundred
// cycles flood the fabric.
ZK_DEV uint64_t ft_wait_prev(const uint64_t* lbw, int64_t t) {
  uint64_t x;
  int nap = 0;
  const uint64_t t_w = wall_clock64();
  for (;;) {
    x = lb_load(&lbw[2 * (t - 1)]);
    if (x != 0) break;
    if (wall_clock64() - t_w > FT_WAIT_TICKS) break;
    // the tile before usually publishes within a microsecond: short
    // naps first (128 cycles), then back off
    if (nap < 16) __builtin_amdgcn_s_sleep(2);
    else if (nap < 32) __builtin_amdgcn_s_sleep(8);
    else __builtin_amdgcn_s_sleep(32);
    ++nap;
  }
  return x;
}

// The entry among the tile before's candidates (lane s < 5: candidate s at
// tile position e, `has` it, its outcome xe in this tile): the first whose
// chain survives — its root word to wE, known: the map answered it (not
// `open`) — else the first one; -1 without any.
ZK_DEV int64_t ft_pick(int64_t ts, bool has, int32_t e, int64_t xe,
                       uint32_t we, bool open, uint32_t& wE, bool& known) {
  const uint64_t hm = __ballot(has);
  const uint64_t lm = __ballot(has && xe != FC_DEAD);
  if (lm) {
    const int l = (int)__builtin_ctzll(lm);
    wE = (uint32_t)__builtin_amdgcn_readlane((int)we, l);
    known = !__builtin_amdgcn_readlane((int)open, l);
    return ts + __builtin_amdgcn_readlane(e, l);
  }
  // no live candidate: the first one
  return hm ? ts + __builtin_amdgcn_readlane(e, (int)__builtin_ctzll(hm)) : -1;
}

// The survivor bits (the map of its frame starts over the tile's positions)
// from its list of m starts, at(i) the i-th.
template <typename At>
ZK_DEV void ft_survivor_bits(uint32_t* sbits, int32_t m, int lane, At at) {
  for (int k = lane; k < FT_SLOT_B / 4; k += 64) sbits[k] = 0u;
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < m; i += 64) {
    const uint32_t q = at(i);
    __hip_atomic_fetch_or(&sbits[q >> 5], 1u << (q & 31), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  __builtin_amdgcn_wave_barrier();
}

// What fs_tile's steps 2-5 need from the kernel.
struct FtCtx {
  const uint8_t* buf;
  uint16_t* list;
  uint16_t* pre;
  int64_t* sx;
  uint64_t* lbw;
  int64_t* rec_entry;
  int64_t* rec_exit;
  int64_t* rec_meta;
  int32_t* rcount;
  int64_t* dbg;
  int64_t* cx;
  uint64_t* stats;
  uint8_t* sb;
  FtBlk blk;
  uint32_t* pk;
  uint16_t* pos;
  uint16_t* slot;
  uint32_t* sbits;
  uint32_t* xbits;
  int64_t n, t, ts, tend, t_0, t_s, t_d;
  int32_t nrel, maxp32, minb, N, misspec;
  bool nospec;
  int lane;
};

// The join: the chain from the entry E walked through the staged tile C.t
// until it meets the survivor's path (C.sbits; its m starts end with code
// send), dies or leaves the tile; the starts walked go to the tile's `pre`.
ZK_DEV void ft_join(const FtCtx& C, int64_t E, int32_t m, int64_t send,
                    FcWalk& wk) {
  const int lane = C.lane;
  const uint8_t* sb = C.sb;
  const int64_t n = C.n, ts = C.ts;
  const int32_t nrel = C.nrel, maxp32 = C.maxp32;
  int64_t c = E;
  uint16_t* P = C.pre + C.t * FT_LMAX;
  int32_t np = 0;
  uint32_t ent = 0;
  for (;;) {
    if (c >= C.tend) { wk.exit = c; break; }
    if (c >= n) { wk.exit = n; break; }  // the stream ends cleanly
    const int32_t crel = (int32_t)(c - ts);
    const uint32_t smw = C.sbits[crel >> 5];
    const int32_t lraw = lds_be32(sb, crel);
    if ((smw >> (crel & 31)) & 1u) {
      // joined: the rest is the survivor's list from this start on
      wk.js = ft_starts_below(C.sbits, crel, lane);
      break;
    }
    const int32_t len = __builtin_amdgcn_readfirstlane(lraw);
    const int32_t nx = crel + 4 + len;
    if ((uint32_t)len > (uint32_t)maxp32 || nx > nrel) {
      wk.exit = c;
      wk.term = true;
      wk.bad = (crel + 4 <= nrel) && ((len < 0) | (len > maxp32));
      break;
    }
    ft_record(P, np, ent, crel, lane);
    c = ts + nx;
  }
  if (lane < (np & 63)) P[(np & ~63) + lane] = (uint16_t)ent;
  wk.np = np;
  wk.cnt = np;
  if (wk.js >= 0) {
    wk.cnt = np + (m - wk.js);
    fc_join_end(wk, send, n);
  }
}

// Tile t's record (fs_link and the rows read it): the survivor's end code
// and start count, the entry used (-1: none) and the walk's result.
// (_lane: written by the calling lane, one tile a lane)
ZK_DEV void ft_put_record_lane(const FtCtx& C, int64_t t, int64_t send,
                               int32_t m, int64_t entry, const FcWalk& wk) {
  C.sx[t] = send;
  C.rcount[t] = m;
  C.rec_entry[t] = entry;
  C.rec_exit[t] = wk.exit;
  C.rec_meta[t] = fc_meta(wk);
}
ZK_DEV void ft_put_record(const FtCtx& C, int64_t t, int64_t send, int32_t m,
                          int64_t entry, const FcWalk& wk) {
  if (C.lane == 0) ft_put_record_lane(C, t, send, m, entry, wk);
}

// The record of the wave's mapped tile C.t and its ZKMI_FS_DBG row: the
// clocks (start, candidates out, entry known, now, nodes found, staged, map
// built), the node count, the jumping rounds and whether the map had the
// entry's chain.
ZK_DEV void ft_put_mapped(const FtCtx& C, int64_t send, int32_t m,
                          int64_t entry, const FcWalk& wk, int64_t t_1,
                          int64_t t_2, int64_t t_f, int rounds, bool done) {
  ft_put_record(C, C.t, send, m, entry, wk);
  if (C.lane == 0 && C.dbg) {
    int64_t* d = C.dbg + 8 * C.t;
    d[0] = C.t_0;
    d[1] = t_1;
    d[2] = t_2;
    d[3] = wall_clock64();
    d[4] = C.t_d;
    d[5] = (int64_t)C.N | (int64_t)rounds << 16 | (int64_t)done << 24;
    d[6] = C.t_s;
    d[7] = t_f;
  }
}

template <int W, bool LONG, int NK>
ZK_DEV int64_t fs_tile_rest(const FtCtx& cx_, bool mapped) {
  const FtCtx& C = cx_;
  const int lane = C.lane;
  const uint8_t* sb = C.sb;
  const int64_t n = C.n, t = C.t, ts = C.ts, tend = C.tend;
  const int32_t nrel = C.nrel, maxp32 = C.maxp32, minb = C.minb;
  constexpr int XW = W / 32;                // candidate words used
  FtNodes<NK> me;
  int rounds = 0;
  if (mapped)
    rounds = ft_build<NK>(me, sb, C.blk, C.pk, C.pos, C.N, nrel, maxp32, minb,
                          lane);
  // the positions are in registers now: R becomes the slots / bits
  for (int k = lane; k < FT_R_B / 4; k += 64) C.sbits[k] = 0u;
  __builtin_amdgcn_wave_barrier();
  const int64_t t_f = C.dbg ? wall_clock64() : 0;

  // ---- 3. the window entries' exits: this tile's candidates for the next -
  int32_t px = -1, sp = -1;
  {
    int32_t x = -1;
    sp = mapped ? ft_cands<W, LONG, NK>(me, sb, C.xbits, x)
                : ft_cands_walk<W>(sb, C.blk, C.xbits, nrel, maxp32, x, lane);
    if (sp >= 0 && x >= 0 && x < (LONG ? FT_S - 1 : W)) px = x;
  }
  // Candidates go out packed in ONE 64-bit word (a relaxed agent-scope
  // store: no fence, no L2 write-back on this multi-XCD part): bit 63 =
  // ready, five 12-bit slots of offset + 1 (0 = empty), slot 0 the preferred
  // one, then up to four other in-window exits in offset order.
  __builtin_amdgcn_wave_barrier();
  uint64_t word = (uint64_t)1 << 63;
  if (px >= 0) word |= (uint64_t)(px + 1);
  {
    uint32_t xw = lane < XW ? C.xbits[lane] : 0u;
    if (px >= 0 && px < W && lane == (px >> 5)) xw &= ~(1u << (px & 31));
    uint64_t any = __ballot(xw != 0);
    int nsl = 1;
    if (px < 0 && any) {
      // no preferred exit: the first in-window one
      const int wl = (int)__builtin_ctzll(any);
      const uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)xw, wl);
      const int x0 = wl * 32 + (int)__builtin_ctz(bits);
      word |= (uint64_t)(x0 + 1);
      if (lane == wl) xw &= ~(1u << (x0 & 31));
      any = __ballot(xw != 0);
    }
    while (any && nsl < 5) {
      const int wl = (int)__builtin_ctzll(any);
      uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)xw, wl);
      while (bits && nsl < 5) {
        const int bit = (int)__builtin_ctz(bits);
        bits &= bits - 1;
        word |= (uint64_t)(wl * 32 + bit + 1) << (12 * nsl);
        ++nsl;
      }
      any &= any - 1;
    }
  }
  if (lane == 0) lb_store(&C.lbw[2 * t], word);    // 0 = not yet
  const int64_t t_1 = C.dbg ? wall_clock64() : 0;

  // ---- 4. the entry: the tile before's candidates, checked in the map ----
  int64_t E = 0;
  bool none = false;
  uint32_t wE = 0;               // the entry's root word, when wE_ok
  bool wE_ok = false;
  if (t > 0 && C.nospec) {
    // (tests: every tile but the first without a speculated entry, the
    // worst case of the link repair; no candidate exits either)
    none = true;
    if (lane < 5) C.cx[5 * t + lane] = FC_DEAD;
  } else if (t > 0) {
    const uint64_t x = ft_wait_prev(C.lbw, t);
    // The first candidate whose chain survives this tile is the entry (a
    // garbage exit of the tile before dies on a bad length here).  Every
    // candidate's outcome goes to `cx`: where two chains both survive tile
    // after tile (a phantom chain), fs_link's chase follows the exact one
    // through this map instead of re-walking every tile.  Lane s checks
    // candidate s in the map; chains the map leaves open are walked.
    const int32_t v = lane < 5 ? (int32_t)((x >> (12 * lane)) & 0xFFF) : 0;
    const bool has = v != 0 && ts + (v - 1) < n;
    const int32_t e = v - 1;
    uint32_t we = 0;
    if (has && mapped) we = ft_root_at(sb, C.blk, C.pk, e, nrel, maxp32, minb);
    const bool open = has && (!mapped || rk_kind(we) == RK_SHORT);
    int64_t xe = has && !open ? ft_cx(sb, we, ts) : FC_DEAD;
    for (uint64_t um = __ballot(open); um; um &= um - 1) {
      const int l = (int)__builtin_ctzll(um);
      const int32_t el = __builtin_amdgcn_readlane(e, l);
      const int64_t r = ft_cand(sb, C.sbits, el, nrel, maxp32, -1, n, ts, 0,
                                lane);
      if (lane == l) xe = r;
    }
    if (lane < 5) C.cx[5 * t + lane] = xe;
    E = ft_pick(ts, has, e, xe, we, open, wE, wE_ok);
    wE_ok = wE_ok && mapped;
    // (tests: every misspec-th tile takes a garbage entry one byte past the
    // chosen one, the link repair's adversary)
    if (C.misspec > 0 && t % C.misspec == 1 && E >= 0 && E + 1 < n) {
      ++E;
      wE_ok = false;
    }
    none = E < 0;
  }
  const int64_t t_2 = C.dbg ? wall_clock64() : 0;

  // ---- 5. the chain's frame starts ---------------------------------------
  // The entry's chain when the map has it (the usual case: its starts are
  // the tile's list, no walk); otherwise the preferred chain's starts are
  // the survivor list (fs_link's repair joins it) and the entry is walked
  // serially until it joins it, dies or leaves, as round 3 did.
  uint16_t* L = C.list + t * FT_LMAX;
  FcWalk wk{E, 0, 0, -1, false, false};
  int64_t send = -1;
  int32_t m = 0;
  bool done = false;
  const int32_t erel = (int32_t)(E - ts);
  if (!none && erel >= nrel) {
    // the entry is the stream's end
    send = TERM | E;
    fc_join_end(wk, send, n);
    done = true;
  } else if (!none && mapped) {
    const uint32_t we = wE_ok ? wE
                              : ft_root_at(sb, C.blk, C.pk, erel, nrel, maxp32,
                                           minb);
    const int32_t D = ft_chain<NK>(me, sb, C.blk, C.slot, erel, we, lane);
    if (D >= 0) {
      for (int32_t k = lane; k < D; k += 64) L[k] = C.slot[k];
      m = D;
      send = ft_send(sb, we, ts);
      wk.cnt = D;
      wk.js = D > 0 ? 0 : -1;
      fc_join_end(wk, send, n);
      done = true;
    }
  }
  if (!done) {
    // survivor list: the preferred chain's starts (from the map, or
    // walked when the tile has none)
    if (sp >= 0 && mapped) {
      const uint32_t ws = ft_root_at(sb, C.blk, C.pk, sp, nrel, maxp32, minb);
      const int32_t D = ft_chain<NK>(me, sb, C.blk, C.slot, sp, ws, lane);
      if (D > 0) {
        for (int32_t k = lane; k < D; k += 64) L[k] = C.slot[k];
        m = D;
        send = ft_send(sb, ws, ts);
      }
    } else if (sp >= 0) {
      __builtin_amdgcn_wave_barrier();
      int32_t last = 0;
      bool run;
      send = ft_walk(sb, sp, nrel, maxp32, ts, L, m, lane, last, run);
      if (m == 0) send = -1;
    }
    __builtin_amdgcn_wave_barrier();
    // survivor bits from the list just stored (each lane rereads only what
    // it wrote itself)
    ft_survivor_bits(C.sbits, m, lane, [&](int i) { return (uint32_t)L[i]; });
    if (!none) {
      // join: walk from the entry until the survivor's path
      ft_join(C, E, m, send, wk);
    } else {
      // no speculated entry: the exit recorded is the survivor's (the
      // likely one), so fs_link's grid repair of the NEXT tile can start
      // from it in the same round as this tile's own repair
      if (m > 0) fc_join_end(wk, send, n);
      if (lane == 0) fc_stat(C.stats, 1, 1), fc_stat(C.stats, LW_NOSPEC, 1);
    }
  }
  ft_put_mapped(C, send, m, none ? -1 : E, wk, t_1, t_2, t_f, rounds, done);
  return send;
}

// ---- tile groups: the map once, then the chain walked on ------------------
// A group of G consecutive tiles is one wave's work (G > 1: streams whose
// frames are large, so a tile holds few of them).  The group's first tile
// gets the chain map as above; its preferred chain is then WALKED through
// the group's other tiles (staged one after the other into the same LDS;
// the next tile's bytes ride in registers while the walk runs), one
// dependent LDS hop per frame: ~20 hops a tile on 192-byte frames, where a
// map costs ~6 us of detection and jumping.  Only the group's first tile
// speculates an entry; the others' entries are the walk's exits, recorded
// as their only candidate (word + cx) so fs_link's chase sees the usual
// maps.  After its walk the group publishes its last exit and takes the
// group before's: the first tile's candidates are checked in a register
// table of its window positions' roots, kept from the map.

// The candidate-exit value of a walk that ended with code `send` after m
// frame starts.
ZK_DEV int64_t ft_cx_of(int64_t send, int32_t m) {
  if (!(send & TERM)) return send | ((int64_t)m << CX_SHIFT);
  return (send & TBAD) ? FC_DEAD : FC_LIVE;
}

// ---- a run of equal frames, taken by gather --------------------------------
// The chain enters tile tk at c after two frames of S bytes.  If the run
// goes on, its frames start at c + j S: lane l reads the length words of
// frames l, l + 64, ... straight from global memory (FT_NGI loads, all
// issued before the first wait; a word not wholly inside the stream is not
// loaded), and the leading frames whose word repeats the length, that end
// inside the stream, are by induction what the hop-by-hop walk finds.  The
// tiles that prefix covers whole get the records the staged walk writes,
// computed (zk_run_span.h): none of their 4 KiB is staged, and a 192-byte
// reply costs one 64-byte sector, not three.  Returns the tiles covered (0:
// the caller walks tile tk: a false trigger costs this one round trip); `send`
// the chain's exit from the last of them; `full`: every word asked for was
// accepted and the group has frames left (gather again).
constexpr int FT_NGI = 4;
static_assert(RUN_TILE == FT_S, "zk_run_span.h: the tile");
struct FtGather {
  uint32_t w[FT_NGI];          // this lane's words: frames lane + 64 i
  int32_t crel, S, room, want, nrel;
  int64_t g_0;
};
// (issued apart from ft_gather_take: the caller puts work under the loads)
ZK_DEV FtGather ft_gather_issue(const FtCtx& C, int64_t c, int32_t S,
                                int64_t tk, int64_t gend) {
  FtGather g;
  const int64_t tsk = tk * FT_S;
  // (wave-uniform: the position and the size in SGPRs)
  g.crel = __builtin_amdgcn_readfirstlane((int32_t)(c - tsk));
  g.S = __builtin_amdgcn_readfirstlane(S);
  g.g_0 = C.dbg ? wall_clock64() : 0;
  g.room = (int32_t)(gend - tk);
  g.nrel = (int32_t)min(C.n - tsk, (int64_t)1 << 30);
  g.want = run_want(g.crel, g.S, g.room * FT_S, 64 * FT_NGI);
  const uint8_t* tb = C.buf + tsk;
#pragma unroll
  for (int i = 0; i < FT_NGI; ++i) {
    const int32_t j = C.lane + 64 * i;
    const int32_t prel = g.crel + j * g.S;
    g.w[i] = 0;
    if (j < g.want && run_word_in(prel, g.nrel))
      __builtin_memcpy(&g.w[i], tb + prel, 4);
  }
  return g;
}
ZK_DEV int32_t ft_gather_take(const FtCtx& C, const FtGather& g, int64_t tk,
                              int64_t& send, bool& full) {
  const int lane = C.lane;
  const int64_t n = C.n, tsk = tk * FT_S;
  const int32_t crel = g.crel, S = g.S, want = g.want, room = g.room;
  const uint32_t(&w)[FT_NGI] = g.w;
  const int64_t g_0 = g.g_0;
  const int64_t g_1 =
      C.dbg ? (__builtin_amdgcn_s_waitcnt(0), wall_clock64()) : 0;
  int32_t a = 0;
  bool open = true;
#pragma unroll
  for (int i = 0; i < FT_NGI; ++i) {
    const int32_t j = lane + 64 * i;
    const int32_t prel = crel + j * S;
    const bool acc = j < want && run_word_in(prel, g.nrel) &&
                     run_accept((int32_t)bswap32(w[i]), S, prel, g.nrel,
                                C.maxp32);
    const uint64_t no = ~__ballot(acc);
    const int32_t ai = no ? (int32_t)__builtin_ctzll(no) : 64;
    a += open ? ai : 0;
    open = open && ai == 64;
  }
  full = a == 64 * FT_NGI;
  const int32_t cov = min(run_tiles_covered(crel, S, a), room);
  if (cov == 0) return 0;
  const int64_t g_2 = C.dbg ? wall_clock64() : 0;
  // the tiles' records, one lane a tile
  int32_t rfirst = 0;
  if (lane < cov) {
    const RunTile r = run_tile(crel, S, a, lane);
    rfirst = r.first;
    const int64_t tq = tk + lane;
    const int64_t entry = tsk + r.entry, exit = tsk + r.exit;
    FcWalk wk{entry, r.count, 0, r.count > 0 ? 0 : -1, false, false};
    fc_join_end(wk, exit, n);
    ft_put_record_lane(C, tq, exit, r.count, entry, wk);
    lb_store(&C.lbw[2 * (tq - 1)],
             (uint64_t)1 << 63 | (uint64_t)(entry - tq * FT_S + 1));
    C.cx[5 * tq] = ft_cx_of(exit, r.count);
#pragma unroll
    for (int s = 1; s < 5; ++s) C.cx[5 * tq + s] = FC_DEAD;
    if (C.dbg) {
      // (dbg: a gathered tile's row — the gather's issue, its arrival, the
      // prefix known, the records)
      int64_t* const dk = C.dbg + 8 * tq;
      dk[0] = g_0;
      dk[1] = g_1;
      dk[2] = g_2;
      dk[3] = wall_clock64();
      dk[5] = (int64_t)r.count;
    }
  }
  // the frame starts: one lane a frame, into its tile's list (the tile's
  // first frame from the lane that wrote its record)
#pragma unroll
  for (int i = 0; i < FT_NGI; ++i) {
    const int32_t j = lane + 64 * i;
    const int32_t prel = crel + j * S;
    const int32_t q = prel >> 12;
    // (the shuffle with every lane active: it reads lane q's register)
    const int32_t first = __shfl(rfirst, q & 63, 64);
    if (j < a && q < cov) {
      C.list[(tk + q) * FT_LMAX + (j - first)] = (uint16_t)(prel & (FT_S - 1));
    }
  }
  send = tsk + run_tile(crel, S, a, cov - 1).exit;
  return cov;
}

// The group's other tiles: the chain leaving tile t0 (end code send0; alive:
// the tile has one; last / run: its last frame's size and whether the frame
// before had it too) followed through them — a run of equal frames by
// gather, anything else walked through the staged tile — each tile's
// records and its one candidate entry written as it goes; then the group's
// last exit published as the next group's candidate.  `nxt` holds tile
// t0 + 1, loaded by the caller (its load overlaps the caller's work); a
// walked tile loads the one after it under its walk, a gathered one loads
// nothing.
template <int W, int G>
ZK_DEV void ft_group_tail(const FtCtx& C, int64_t send0, bool alive,
                          FtTileRegs& nxt, int32_t last, bool run) {
  const int lane = C.lane;
  uint8_t* sb = C.sb;
  const int64_t n = C.n, t0 = C.t;
  const int32_t maxp32 = C.maxp32;
  const int64_t ntiles = (n + FT_S - 1) / FT_S;
  const int64_t gend = min(t0 + G, ntiles);
  int64_t send = send0;
  int32_t kdone = 1;
  int k = 1;
  // ---- a run leaving tile t0: taken by gather, round after round ---------
  // (tile t0 + 1, which nxt holds, goes to LDS under the first gather: the
  // walk's, should the run break in it)
  // (the 256-byte window's instances only: with the 512-byte window's
  // larger entry table the gather's registers cost the third wave a SIMD.
  // The 256-byte ones stand at 163 VGPRs with it, 5 below the 168 that 3
  // waves a SIMD allow: check tools/kernel_resources.py after any change to
  // the grouped path, profiles/run_gather_resources.md)
  if (W <= 256 && run && last >= 16 && last <= FT_S && t0 + 1 < ntiles &&
      alive && !(send & TERM)) {
    bool full = true, first = true;
    while (full && k < G && t0 + k < ntiles && send >= (t0 + k) * FT_S &&
           send < (t0 + k + 1) * FT_S) {
      const FtGather g = ft_gather_issue(C, send, last, t0 + k, gend);
      if (first) ft_store(sb, nxt, lane);
      first = false;
      const int32_t cov = ft_gather_take(C, g, t0 + k, send, full);
      if (cov == 0) break;
      k += cov;
    }
    kdone = k;
    // (the tile the run ends in: its bytes on demand.  No tile rides in
    // registers while a gather is taken, so a run that ends in tile t0 + 1
    // loads that tile again, from L2)
    if (k < G && t0 + k < ntiles)
      ft_load(C.buf, n, (t0 + k) * FT_S, lane, nxt);
  }
  // ---- the group's other tiles: the survivor's chain walked on -----------
  for (; k < G; ++k) {
    const int64_t tk = t0 + k;
    if (tk >= ntiles) break;
    const int64_t tsk = tk * FT_S;
    const int64_t c = send;                 // the chain's entry into tk
    const bool live = alive && !(send & TERM) && c >= tsk &&
                      c < tsk + FT_S;
    if (!live) break;
    // (dbg: a walked tile's row holds its clocks — before the store, after
    // it (the load's wait), after the walk, after the records)
    int64_t* const dk = C.dbg ? C.dbg + 8 * tk : nullptr;
    const int64_t k_0 = dk ? wall_clock64() : 0;
    ft_store(sb, nxt, lane);
    const int64_t k_1 = dk ? wall_clock64() : 0;
    if (k + 1 < G && tk + 1 < ntiles) ft_load(C.buf, n, tsk + FT_S, lane, nxt);
    int32_t m;
    const int32_t nrelk = (int32_t)min(n - tsk, (int64_t)1 << 30);
    send = ft_walk(sb, (int32_t)(c - tsk), nrelk, maxp32, tsk,
                   C.list + tk * FT_LMAX, m, lane, last, run);
    const int64_t k_2 = dk ? wall_clock64() : 0;
    FcWalk wk{c, m, 0, m > 0 ? 0 : -1, false, false};
    fc_join_end(wk, send, n);
    ft_put_record(C, tk, send, m, c, wk);
    if (lane == 0) {
      // the tile's one candidate entry: the walk's (for fs_link's chase)
      lb_store(&C.lbw[2 * (tk - 1)],
               (uint64_t)1 << 63 | (uint64_t)(c - tsk + 1));
      C.cx[5 * tk] = ft_cx_of(send, m);
      if (dk) {
        dk[0] = k_0;
        dk[1] = k_1;
        dk[2] = k_2;
        dk[3] = wall_clock64();
        dk[5] = (int64_t)m;
      }
    }
    if (lane >= 1 && lane < 5) C.cx[5 * tk + lane] = FC_DEAD;
    kdone = k + 1;
  }
  // tiles the walk did not reach: no entry (fs_link re-walks them)
  for (int k = kdone; k < G; ++k) {
    const int64_t tk = t0 + k;
    if (tk >= ntiles) break;
    if (lane == 0) lb_store(&C.lbw[2 * (tk - 1)], (uint64_t)1 << 63);
    ft_put_record(C, tk, -1, 0, -1, FcWalk{-1, 0, 0, -1, false, false});
    if (lane < 5) C.cx[5 * tk + lane] = FC_DEAD;
  }
  // the group's last exit: the next group's candidate
  const int64_t tl = min(t0 + G, ntiles) - 1;
  {
    uint64_t word = (uint64_t)1 << 63;
    const int64_t tle = (tl + 1) * FT_S;
    if (kdone == (int32_t)(tl - t0 + 1) && alive && !(send & TERM) &&
        send >= tle && send < tle + W)
      word |= (uint64_t)(send - tle + 1);
    if (lane == 0) lb_store(&C.lbw[2 * tl], word);
  }
}

template <int W, int NK, int G>
ZK_DEV void fs_group_rest(const FtCtx& cx_) {
  static_assert(G > 1 && W <= 512, "groups: small windows");
  constexpr int WJ = W / 64;                // window positions per lane
  const FtCtx& C = cx_;
  const int lane = C.lane;
  uint8_t* sb = C.sb;
  const int64_t n = C.n, t0 = C.t, ts = C.ts;
  const int32_t nrel = C.nrel, maxp32 = C.maxp32, minb = C.minb;
  const int64_t ntiles = (n + FT_S - 1) / FT_S;
  FtNodes<NK> me;
  const int rounds = ft_build<NK>(me, sb, C.blk, C.pk, C.pos, C.N, nrel,
                                  maxp32, minb, lane);
  for (int k = lane; k < FT_R_B / 4; k += 64) C.sbits[k] = 0u;
  __builtin_amdgcn_wave_barrier();
  const int64_t t_f = C.dbg ? wall_clock64() : 0;

  // ---- the first tile: its preferred chain (the survivor) and its window
  // positions' roots, in registers for the entry check after the walk
  int32_t x = -1;
  const int32_t sp = ft_cands<W, false, NK>(me, sb, C.xbits, x);
  uint32_t rw[WJ];
  int64_t rx[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    const int32_t e = lane + 64 * j;
    rw[j] = e < nrel ? ft_root_at(sb, C.blk, C.pk, e, nrel, maxp32, minb)
                     : rk(RK_END, 0, 0);
    rx[j] = e < nrel ? ft_cx(sb, rw[j], ts) : FC_LIVE;
  }
  int32_t m0 = 0;
  int64_t send0 = -1;
  uint32_t ws = 0;
  uint16_t* L0 = C.list + t0 * FT_LMAX;
  if (sp >= 0) {
    ws = ft_root_at(sb, C.blk, C.pk, sp, nrel, maxp32, minb);
    const int32_t D = ft_chain<NK>(me, sb, C.blk, C.slot, sp, ws, lane);
    if (D >= 0) {
      for (int32_t k = lane; k < D; k += 64) L0[k] = C.slot[k];
      m0 = D;
      send0 = ft_send(sb, ws, ts);
    } else {
      // (a side branch or a short frame on it: walked)
      __builtin_amdgcn_wave_barrier();
      int32_t last = 0;
      bool run;
      send0 = ft_walk(sb, sp, nrel, maxp32, ts, L0, m0, lane, last, run);
      for (int32_t k = lane; k < m0; k += 64) C.slot[k] = L0[k];
      ws = 0;                  // (the slots hold the walk's starts)
    }
  }
  // the survivor's starts move to the node words' LDS, which nothing reads
  // after the map (R becomes the survivor bits if tile t0 has to come back;
  // in registers they were 6 VGPRs carried across the whole tail)
  static_assert(FT_SLOTS * 2 <= FT_NMAX * 4, "the starts fit the node words");
  __builtin_amdgcn_wave_barrier();
  uint16_t* const sv = (uint16_t*)C.pk;
  for (int32_t k = lane; k < m0; k += 64) sv[k] = C.slot[k];
  __builtin_amdgcn_wave_barrier();
  // the run state the tail starts from: the chain's last frame's size, and
  // whether the frame before had it too
  int32_t last0 = 0;
  bool run0 = false;
  if (m0 >= 1 && send0 >= 0 && !(send0 & TERM)) {
    const int32_t a = __builtin_amdgcn_readfirstlane(sv[m0 - 1]);
    const int32_t b = __builtin_amdgcn_readfirstlane(sv[m0 >= 2 ? m0 - 2 : 0]);
    last0 = (int32_t)(send0 - ts) - a;
    run0 = m0 >= 2 && a - b == last0;
  }
  const int64_t t_1 = C.dbg ? wall_clock64() : 0;

  FtTileRegs nxt;
  if (G > 1 && t0 + 1 < ntiles) ft_load(C.buf, n, ts + FT_S, lane, nxt);
  ft_group_tail<W, G>(C, send0, sp >= 0, nxt, last0, run0);

  // ---- the first tile's entry: the group before's exit -------------------
  int64_t E = 0;
  bool none = false;
  uint32_t wE = 0;
  bool known = false;          // wE / the candidate values from the table
  bool staged = false;         // tile t0 back in LDS (the fallbacks)
  auto restage = [&]() {
    if (staged) return;
    FtTileRegs r;
    ft_load(C.buf, n, ts, lane, r);
    ft_store(sb, r, lane);
    // survivor bits from the survivor's starts
    ft_survivor_bits(C.sbits, m0, lane,
                     [&](int i) { return (uint32_t)sv[i]; });
    staged = true;
  };
  if (t0 > 0 && C.nospec) {
    // (tests: no group takes a speculated entry, as fs_tile_rest)
    none = true;
    if (lane < 5) C.cx[5 * t0 + lane] = FC_DEAD;
  } else if (t0 > 0) {
    const uint64_t xw = ft_wait_prev(C.lbw, t0);
    // lane s: candidate s, looked up in the window table (the lane owning
    // position e holds its root in register e / 64)
    const int32_t v = lane < 5 ? (int32_t)((xw >> (12 * lane)) & 0xFFF) : 0;
    const bool has = v != 0 && ts + (v - 1) < n;
    const int32_t e = v - 1;
    uint32_t we = 0;
    int64_t xe = FC_DEAD;
    bool open = false;
    for (int s = 0; s < 5; ++s) {
      const int32_t es = __builtin_amdgcn_readlane(e, s);
      if (!__builtin_amdgcn_readlane((int)has, s)) continue;
      if (es >= W) {
        if (lane == s) open = true;
        continue;
      }
      const int jj = es >> 6, ll = es & 63;
      uint32_t wv = 0;
      int64_t xv = 0;
#pragma unroll
      for (int j = 0; j < WJ; ++j)
        if (j == jj) { wv = rw[j]; xv = rx[j]; }
      const uint32_t wsv = (uint32_t)__builtin_amdgcn_readlane((int)wv, ll);
      const int64_t xsv = (int64_t)(
          (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)xv,
                                                         ll) |
          (uint64_t)(uint32_t)__builtin_amdgcn_readlane(
              (int)(uint32_t)((uint64_t)xv >> 32), ll) << 32);
      if (lane == s) {
        we = wsv;
        xe = xsv;
        open = rk_kind(wsv) == RK_SHORT;
      }
    }
    if (__ballot(open)) {
      restage();
      for (uint64_t um = __ballot(open); um; um &= um - 1) {
        const int l = (int)__builtin_ctzll(um);
        const int32_t el = __builtin_amdgcn_readlane(e, l);
        const int64_t r = ft_cand(sb, C.sbits, el, nrel, maxp32, send0, n,
                                  ts, m0, lane);
        if (lane == l) xe = r;
      }
    }
    if (lane < 5) C.cx[5 * t0 + lane] = xe;
    E = ft_pick(ts, has, e, xe, we, open, wE, known);
    // (tests: every misspec-th group takes a garbage entry one byte past the
    // chosen one, as fs_tile_rest's tiles do)
    if (C.misspec > 0 && (t0 / G) % C.misspec == 1 && E >= 0 && E + 1 < n) {
      ++E;
      known = false;
    }
    none = E < 0;
  } else {
    wE = rw[0];                 // lane 0's position 0
    wE = (uint32_t)__builtin_amdgcn_readlane((int)wE, 0);
    known = true;
  }
  const int64_t t_2 = C.dbg ? wall_clock64() : 0;

  // ---- the first tile's records -------------------------------------------
  FcWalk wk{E, 0, 0, -1, false, false};
  const int32_t erel = (int32_t)(E - ts);
  bool done = false;
  if (!none && erel >= nrel) {
    fc_join_end(wk, TERM | E, n);
    done = true;
  } else if (!none && known && ws != 0 && (wE >> 16) == (ws >> 16) &&
             (int32_t)rk_cnt(wE) <= m0 && rk_cnt(wE) > 0 &&
             __builtin_amdgcn_readfirstlane(
                 (int32_t)sv[m0 - (int32_t)rk_cnt(wE)]) == erel) {
    // the entry is on the survivor's chain: the rest is its list
    wk.js = m0 - (int32_t)rk_cnt(wE);
    wk.cnt = (int32_t)rk_cnt(wE);
    fc_join_end(wk, send0, n);
    done = true;
  }
  if (!done && !none) {
    // join: walk from the entry (tile t0 back in LDS) until the survivor's
    // path, as a single tile does
    restage();
    ft_join(C, E, m0, send0, wk);
  } else if (none) {
    if (m0 > 0) fc_join_end(wk, send0, n);
    if (lane == 0) fc_stat(C.stats, 1, 1), fc_stat(C.stats, LW_NOSPEC, 1);
  }
  ft_put_mapped(C, send0, m0, none ? -1 : E, wk, t_1, t_2, t_f, rounds, done);
}

template <int W, bool LONG, int G>
__global__ __launch_bounds__(256) void fs_tile(
    const uint8_t* __restrict__ buf, const int64_t* __restrict__ n_dev,
    int64_t n_cap, int64_t maxp, uint16_t* __restrict__ list,
    uint16_t* __restrict__ pre, int64_t* __restrict__ sx, uint64_t* lbw,
    int64_t* __restrict__ rec_entry, int64_t* __restrict__ rec_exit,
    int64_t* __restrict__ rec_meta, int32_t* __restrict__ rcount,
    int64_t ntiles_cap, int64_t* __restrict__ dbg, int32_t minb,
    int32_t tflags, int64_t* __restrict__ cx) {
  static_assert(W % 64 == 0 && W <= 2048, "window");
  // one tile per wave; a block's waves work independently (no barriers),
  // each in its own LDS slice
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_all[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* smem = smem_all + wv * FT_LDS;
  FtCtx C;
  C.sb = smem;
  uint64_t* bmask = (uint64_t*)(smem + FT_O_BLK);
  uint16_t* bbase = (uint16_t*)(smem + FT_O_BASE);
  C.blk.mask = bmask;
  C.blk.base = bbase;
  C.pk = (uint32_t*)(smem + FT_O_PK);
  C.pos = (uint16_t*)(smem + FT_O_R);
  C.slot = (uint16_t*)(smem + FT_O_R);
  C.sbits = (uint32_t*)(smem + FT_O_R);
  C.xbits = (uint32_t*)(smem + FT_O_XB);
  const int lane = threadIdx.x & 63;
  const int64_t n = stream_len(n_dev, n_cap);
  const int64_t ntiles = (n + FT_S - 1) / FT_S;
  // (tiles in workgroup order: a tile's predecessor was dispatched before
  // it.  An XCD-by-XCD mapping — each XCD a contiguous tile range — put
  // the predecessor on the same L2 but started every range's tail later:
  // reply stream 94 -> 103 us.)
  const int64_t t = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wv) * G;
  if (t >= ntiles) return;
  C.t_0 = dbg ? wall_clock64() : 0;
  const int64_t ts = t * FT_S;
  const int64_t tend = ts + FT_S;
  const int32_t nrel = (int32_t)min(n - ts, (int64_t)1 << 30);
  const int32_t maxp32 = (int32_t)maxp;
  uint8_t* sb = C.sb;

  // ---- stage the tile (all loads issued before the first LDS write) ------
  {
    FtTileRegs r;
    ft_load(buf, n, ts, lane, r);
    ft_store(sb, r, lane);
  }
  C.t_s = dbg ? (__builtin_amdgcn_s_waitcnt(0), wall_clock64()) : 0;

  // ---- 1. nodes: lane l tests positions 64l .. 64l + 63 ------------------
  int32_t N;
  {
    const int32_t P0 = lane * 64;
    uint32_t d[17];
    {
      // lane l reads its 16-byte chunks in the order rotated by (l >> 2) & 3:
      // a ds_read_b128 lane group (16 lanes) then covers the 64 banks once
      // (in plain order four lanes share each 16-byte slot: 4-way); the
      // dword past the lane's 64 bytes is the next lane's first (a shuffle,
      // not a 16-way ds_read_b32 at a 64-byte stride)
      const int r = (lane >> 2) & 3;
      uint4 x0 = *(const uint4*)(sb + P0 + 16 * (r & 3));
      uint4 x1 = *(const uint4*)(sb + P0 + 16 * ((1 + r) & 3));
      uint4 x2 = *(const uint4*)(sb + P0 + 16 * ((2 + r) & 3));
      uint4 x3 = *(const uint4*)(sb + P0 + 16 * ((3 + r) & 3));
      const uint32_t pad = *(const uint32_t*)(sb + FT_S);   // (broadcast)
      // back to chunk order (x_j held chunk j + r): rotate right by r in two
      // conditional stages (named registers and selects: an indexed array
      // went to scratch)
      auto sel = [](bool c, uint4 a, uint4 b) {
        return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z,
                          c ? a.w : b.w);
      };
      {
        const bool c = r & 1;
        const uint4 y0 = sel(c, x3, x0), y1 = sel(c, x0, x1),
                    y2 = sel(c, x1, x2), y3 = sel(c, x2, x3);
        x0 = y0; x1 = y1; x2 = y2; x3 = y3;
      }
      {
        const bool c = r & 2;
        const uint4 y0 = sel(c, x2, x0), y1 = sel(c, x3, x1),
                    y2 = sel(c, x0, x2), y3 = sel(c, x1, x3);
        x0 = y0; x1 = y1; x2 = y2; x3 = y3;
      }
      d[0] = x0.x; d[1] = x0.y; d[2] = x0.z; d[3] = x0.w;
      d[4] = x1.x; d[5] = x1.y; d[6] = x1.z; d[7] = x1.w;
      d[8] = x2.x; d[9] = x2.y; d[10] = x2.z; d[11] = x2.w;
      d[12] = x3.x; d[13] = x3.y; d[14] = x3.z; d[15] = x3.w;
      const uint32_t nx = (uint32_t)__shfl_down((int)d[0], 1, 64);
      d[16] = lane == 63 ? pad : nx;
    }
    // minb <= len <= W - 4 past the entry window (the window covers the
    // stream's frames: a longer length is a byte pattern, not a frame; the
    // rare real one meets the map as a SHORT root and is walked exactly),
    // len < FT_LIMIT in long-frame mode; in the entry window any legal
    // length (a frame there longer than the tile is still an entry's
    // chain).  (Length-like words inside frames — zxids in [2^27, 2^28)
    // read 2048..4095 — took a create / set / delete reply tile past
    // FT_NMAX nodes: no map, no speculation, a 200 ms serial repair.)
    const uint32_t lim = P0 < W ? (uint32_t)(maxp32 - minb + 1)
                         : LONG ? (uint32_t)(FT_LIMIT - minb)
                                : (uint32_t)(W - 3 - minb);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const uint32_t v = (uint32_t)be32_of(d[j >> 2], d[(j >> 2) + 1], j);
      lo |= ((v - (uint32_t)minb) < lim ? 1u : 0u) << j;
    }
#pragma unroll
    for (int j = 32; j < 64; ++j) {
      const uint32_t v = (uint32_t)be32_of(d[j >> 2], d[(j >> 2) + 1], j);
      hi |= ((v - (uint32_t)minb) < lim ? 1u : 0u) << (j - 32);
    }
    uint64_t mask = (uint64_t)hi << 32 | lo;
    // a node's length word lies inside the stream
    const int32_t room = nrel - 4 - P0;      // last position with a header
    if (room < 63) mask = room < 0 ? 0 : mask & ((2ull << room) - 1);
    const uint32_t c = (uint32_t)__popcll(mask);
    uint32_t incl = c;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t y = __shfl_up(incl, s, 64);
      if (lane >= s) incl += y;
    }
    N = __builtin_amdgcn_readlane((int)incl, 63);
    const uint32_t base = incl - c;
    bmask[lane] = mask;
    bbase[lane] = (uint16_t)base;
    if (N <= FT_NMAX) {
      uint32_t k = base;
      uint64_t m = mask;
      while (m) {
        C.pos[k++] = (uint16_t)(P0 + __builtin_ctzll(m));
        m &= m - 1;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  C.t_d = dbg ? wall_clock64() : 0;
  C.buf = buf; C.list = list; C.pre = pre; C.sx = sx; C.lbw = lbw;
  C.rec_entry = rec_entry; C.rec_exit = rec_exit; C.rec_meta = rec_meta;
  C.rcount = rcount; C.dbg = dbg; C.cx = cx;
  C.stats = &lbw[2 * ntiles_cap];
  C.n = n; C.t = t; C.ts = ts; C.tend = tend;
  C.nrel = nrel; C.maxp32 = maxp32; C.minb = minb; C.N = N;
  C.nospec = tflags & 1;
  C.misspec = tflags >> 8;
  C.lane = lane;
  // ---- 2-5, with this lane's share of the nodes in registers -------------
  static_assert(FT_NMAX == 512, "node buckets");
  if constexpr (G > 1) {
    static_assert(!LONG, "groups: frames within the window");
    if (N <= 128) fs_group_rest<W, 2, G>(C);
    else if (N <= 256) fs_group_rest<W, 4, G>(C);
    else if (N <= FT_NMAX) fs_group_rest<W, 8, G>(C);
    else {
      // no map for the first tile (its candidates walked lane by lane):
      // its survivor's exit is walked on through the group as usual
      const int64_t s0 = fs_tile_rest<W, LONG, 1>(C, false);
      FtTileRegs nxt;
      if (t + 1 < (n + FT_S - 1) / FT_S) ft_load(buf, n, ts + FT_S, lane, nxt);
      ft_group_tail<W, G>(C, s0, s0 >= 0, nxt, 0, false);
    }
  } else {
    if (N <= 128) fs_tile_rest<W, LONG, 2>(C, true);
    else if (N <= 256) fs_tile_rest<W, LONG, 4>(C, true);
    else if (N <= FT_NMAX) fs_tile_rest<W, LONG, 8>(C, true);
    else fs_tile_rest<W, LONG, 1>(C, false);
  }
}


// ---- the launch (frame_tile.hip, frame_group256.hip, frame_group512.hip) ----

template <int W, bool LONG, int G>
int fs_tile_launch(const TileLaunch& l, hipStream_t st) {
  const FsWs& w = *l.ws;
  const int64_t waves = (w.tiles + G - 1) / G;
  const unsigned blocks = (unsigned)((waves + FS_TPB - 1) / FS_TPB);
  fs_tile<W, LONG, G><<<blocks, 64 * FS_TPB, FT_LDS * FS_TPB, st>>>(
      l.buf, l.n_dev, l.n_cap, l.maxp, w.list, w.pre, w.sx, w.lbw, w.rent,
      w.rexit, w.rmeta, w.rcnt, w.tiles, l.dbg, FS_MINB, l.tflags, w.cx);
  ZK_LAUNCH_CHECK();
  return 0;
}

// The grouped instances of one window (a file each: they are most of K1's
// compile time).
template <int W>
int fs_group_launch(const TileLaunch& l, hipStream_t st) {
  switch (l.G) {
    case 8: return fs_tile_launch<W, false, 8>(l, st);
    case 4: return fs_tile_launch<W, false, 4>(l, st);
    case 2: return fs_tile_launch<W, false, 2>(l, st);
    default: return -1;
  }
}

}  // namespace zk
