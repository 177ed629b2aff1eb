// K1 — parallel length-prefixed frame scan.
//
// Reference: ZKDecodeStream._transform (lib/zk-streams.js:39-65) walks the
// i32-BE length chain one frame at a time and memmoves the remainder per
// packet (O(bytes x packets)).  The chain is inherently
// sequential; we make it parallel over 4 KiB tiles in three launches:
//
//  fs_tile   ONE WAVE per tile (or per group of G = 2 / 4 tiles on streams
//            of large frames), two waves a workgroup, no barriers.  The tile
//            is staged into the wave's LDS once; everything else runs there:
//            1. nodes: every position whose i32-BE word is a plausible
//               length (8 <= len < 4 KiB; any legal length inside the entry
//               window) is a node, found 64 positions a lane;
//            2. the chain map: each node's successor (p + 4 + len) is
//               resolved by POINTER JUMPING over the node table in
//               registers (log2(chain length) rounds, ~5-7 on GET streams),
//               so every node knows where its chain leaves the tile, how
//               many frames it takes and whether it dies (a garbage entry
//               lands on a non-node within a hop or two);
//            3. the tile's candidate entries for the next tile — the exits
//               of the chains rooted in the window — go out in ONE packed
//               64-bit word (ready bit + five 12-bit offsets, a relaxed
//               agent-scope store: no release fence, which costs an L2
//               writeback per wave on a multi-XCD part);
//            4. the entry: the tile before's candidates, each looked up in
//               the map (the first whose chain survives is the entry; every
//               candidate's exit goes to `cx`, the entry -> exit map the
//               repair chases through);
//            5. the entry's chain read out of the map into the tile's list
//               of frame starts (a chain the map left open — a short frame
//               on it — is walked serially, as is a join onto the preferred
//               chain).
//            A group maps its first tile and walks the chain on through the
//            others (one LDS hop a frame), then checks its entry in a
//            register table of the first tile's window roots.
//  fs_link   The check over a grid of 16 workgroups (one wave per 64 tiles:
//            is each tile's entry the exit of the tile before, the first
//            terminal, the in-block frame counts; a launch of its own until
//            round 4 — moving it into fs_tile cost the tiles' ends more than
//            the launch), then a ticket: the LAST block to finish its check
//            goes on alone, no block waits for another (no grid barrier, so
//            no co-residency is assumed).  No broken link before the first
//            terminal (the usual case): it scans the block totals into row
//            bases, done.  Otherwise the repair: a few broken links are
//            chased in parallel waves — from each, forward while the next
//            link stays broken, the exact entry of a tile looked up among
//            the candidates fs_tile mapped (`cx`), so a run of tiles costs a
//            few instructions each; many, or what the chases leave, by the
//            tail: exact chases from the leftmost broken link, tiles whose
//            entry is no candidate walked, tiles covered whole by one frame
//            filled in one step; then the counts are scanned up to the first
//            terminal: row bases and result[0..3].
//            The last block also scatters the frame-block index (for every
//            256 rows, the count block their first row lies in).
//  fs_rows   one wave per tile writes its (body offset, length) rows.
//
// Who writes the rows and clears the flags (zk_frame_rows.h holds the one
// implementation of both):
//  * plain scan: fs_rows writes foff / flen, clears every tile's candidate
//    flags and fs_link's tail words; the next scan of the workspace may run
//    with clean = 1.
//  * rows deferred (flags bit 24, FS_DEFER): fs_tile and fs_link only;
//    result[0..3] are complete, foff / flen untouched.  The table's first
//    reader — decode_replies_tiles_k, tree_serve_tiles_k — takes each
//    workgroup's 256 rows from the tile lists through the index, stores
//    them to foff / flen, and clears the flags (a strided share of the tiles
//    a workgroup, the tail words by workgroup 0).  Only after such a
//    consumer ran may the next scan pass clean = 1; without one it memsets.
//  * a stream of one tile at most: fs_small writes the rows; there are no
//    flags, and no deferred mode.
//
// The stream length is read ON THE DEVICE (n = min(*n_dev, n_cap), e.g. an
// encoder's total): the grids cover the buffer capacity, tiles past the
// length return at once, and no byte past it is read.  BAD_LENGTH is
// reported at the exact frame (result[1] = its offset, result[2] = 1), the
// consumed prefix ends at the last complete frame, and a partial trailing
// frame is left for the next call (carry), like the reference's buffer.
//
// History (profiles/): round 1 scanned 16 KiB tiles with a 256-thread
// frontier block, a separate survivor kernel through a 4 KiB LDS ring, and
// log-depth function composition + push-down + join + count scan + write
// (13-15 launches, ~130 us per 200 MB reply stream on the composition
// alone).  A single-pass decoupled look-back replacing the composition
// stalled: with every tile resident at once, each tile looked back across
// all the tiles before it (~100 us).  The survivor's 2 KiB ring reloads
// stalled on HBM latency at every chunk (~1 us per reply frame).  Staging
// a 4 KiB tile once per wave removes both.
//
// This header is private to the K1 files (frame_scan.hip, frame_tile.hip,
// frame_group256.hip, frame_group512.hip, frame_link.hip); the consumers
// include zk_frame_rows.h.
#pragma once
#include <stddef.h>

#include "zk_common.h"
#include "zk_frame_rows.h"   // tile constants, LW_* words, the rows

namespace zk {

constexpr int64_t TERM = (int64_t)1 << 62;
constexpr int64_t TBAD = (int64_t)1 << 60;
constexpr int64_t FC_MAXP = (int64_t)1 << 24;
constexpr int FC_WIN = 4096;               // fs_link's staged walk window
// fs_link threads (512: 256 VGPRs a lane — with 1024 the chase and the walk
// inlined together spilled to scratch, 0.64 us a looked-up tile)
constexpr int FL_T = 512;
constexpr int FL_U = 8;                    // fs_link loads per batch
constexpr int FL_BROUNDS = 8;             // the last block's repair rounds
constexpr int FL_DBG_BLOCKS = 16;          // fs_link blocks with a debug clock
constexpr int FL_DBG_ROWS = 6;             // fs_link's debug rows past the tiles
// The last block's one exact chase before its rounds (many broken links):
// tiles it may walk before it leaves the rest to the rounds
constexpr uint32_t FL_CHASE_WALKS = 16;
// The big repair (barrier rounds over the grid) when a scan has more tiles
// without a speculated entry than this
constexpr unsigned FL_BIG_NOSPEC = 256;
constexpr int FL_GROUNDS = 6;              // its grid rounds
// Bound of fs_tile's wait for the tile before (100 MHz ticks, 2 ms): normal
// waits are tens of microseconds; past the bound the tile takes no
// speculated entry and fs_link re-walks it from the exact one.
constexpr uint64_t FT_WAIT_TICKS = 200000;

ZK_DEV uint64_t lb_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
ZK_DEV void lb_store(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
ZK_DEV int64_t ld_agent(const int64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
ZK_DEV void st_agent(int64_t* p, int64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Chain statistics after the X flags: [0] tiles fs_link's chases looked up,
// [1] tiles without a speculated entry, [2] tiles re-walked by fs_link, [3]
// fs_link repair rounds (zk_frame_scan_stats reads them).
ZK_DEV void fc_stat(uint64_t* stats, int k, uint32_t v) {
  __hip_atomic_fetch_add((uint32_t*)&stats[k], v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// per-tile record: meta = cnt | np << 11 | (js + 1) << 22 | term << 33 |
// bad << 34; entry = the entry used (-1: none, the tile before had no
// speculated exit); exit = exit position or the terminal's position.
struct FcWalk {
  int64_t exit;
  int32_t cnt;       // frame starts of the tile on the chain
  int32_t np;        // of which walked before meeting the survivor (pre[])
  int32_t js;        // survivor list index the rest starts at (-1: none)
  bool term, bad;
};
ZK_DEV int64_t fc_meta(const FcWalk& w) {
  return (int64_t)w.cnt | ((int64_t)w.np << 11) | ((int64_t)(w.js + 1) << 22) |
         ((int64_t)w.term << 33) | ((int64_t)w.bad << 34);
}
// (the m_* readers and M_STALE: zk_frame_rows.h)

// Resolve the survivor's end code `send` into the walk result's exit.
ZK_DEV void fc_join_end(FcWalk& r, int64_t send, int64_t n) {
  if (send & TERM) {
    const int64_t q = send & ~(TERM | TBAD);
    if (q >= n && !(send & TBAD)) {
      r.exit = n;                           // clean end of the stream
    } else {
      r.exit = q; r.term = true; r.bad = (send & TBAD) != 0;
    }
  } else {
    r.exit = send;
  }
}

// A candidate's outcome in a tile (fs_tile's `cx`, fs_link's chase): the
// absolute exit (>= the tile end) packed with the frames the chain starts
// in the tile (cx_exit / cx_cnt); FC_DEAD when it hits a bad length; FC_LIVE
// when it survives without a known exit (ft_cand, zk_frame_tile.h).
constexpr int64_t FC_DEAD = -1;
constexpr int64_t FC_LIVE = -2;
constexpr int CX_SHIFT = 48;
ZK_DEV int64_t cx_exit(int64_t v) {
  return v < 0 ? v : v & (((int64_t)1 << CX_SHIFT) - 1);
}
ZK_DEV int32_t cx_cnt(int64_t v) { return v < 0 ? 0 : (int32_t)(v >> CX_SHIFT); }

// ---- the host's side --------------------------------------------------------

// The workspace's words after the X flags, by name (LW_* are their indices).
struct FsTail {
  // chain statistics (fc_stat's k, zk_frame_scan_stats)
  uint64_t looked, nospec_total, walked, rounds;
  uint64_t mins[2];                // the check's minima
  int64_t lastk;                   // the last live tile
  uint64_t nospec;                 // this scan's tiles without an entry
  unsigned long long grid[LW_BIG - LW_GRID];   // fs_link's grid words
  unsigned long long big[LW_END - LW_BIG];     // its barrier words
};
static_assert(sizeof(FsTail) == LW_END * 8 &&
              offsetof(FsTail, mins) == LW_MINS * 8 &&
              offsetof(FsTail, lastk) == LW_LAST * 8 &&
              offsetof(FsTail, nospec) == LW_NOSPEC * 8 &&
              offsetof(FsTail, grid) == LW_GRID * 8 &&
              offsetof(FsTail, big) == LW_BIG * 8, "the LW_* words");

// The workspace of a scan over n_cap bytes: every array, typed.  The one
// place that knows the layout (ws null: only tiles / total are meaningful).
struct FsWs {
  int64_t tiles;
  size_t total;
  uint16_t *list, *pre;            // frame starts, FT_LMAX a tile each
  int64_t* sx;                     // the survivor's end code
  uint64_t* lbw;                   // X flags, 2 a tile; then the tail words
  FsTail* tail;
  size_t lbw_bytes;                // flags + tail: what a scan finds zeroed
  int64_t *rent, *rexit, *rmeta;   // the tile records
  int32_t* rcnt;
  int64_t *base, *bsum;            // row bases: in-block, per count block
  int32_t* blist;                  // broken links
  int64_t* cx;                     // candidate exits (fs_tile), 5 a tile
  int32_t* fblk;                   // the frame-block index
};

inline FsWs fs_view(uint8_t* ws, int64_t n_cap) {
  FsWs v{};
  const int64_t tiles = n_cap > 0 ? (n_cap + FT_S - 1) / FT_S : 1;
  v.tiles = tiles;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    uint8_t* r = ws ? ws + o : nullptr;
    o += (bytes + 255) & ~(size_t)255;
    return r;
  };
  v.list = (uint16_t*)take((size_t)tiles * FT_LMAX * 2);
  v.pre = (uint16_t*)take((size_t)tiles * FT_LMAX * 2);
  v.sx = (int64_t*)take((size_t)tiles * 8);
  v.lbw_bytes = (size_t)(2 * tiles) * 8 + sizeof(FsTail);
  v.lbw = (uint64_t*)take(v.lbw_bytes);
  v.tail = ws ? (FsTail*)(v.lbw + 2 * tiles) : nullptr;
  v.rent = (int64_t*)take((size_t)tiles * 8);
  v.rexit = (int64_t*)take((size_t)tiles * 8);
  v.rmeta = (int64_t*)take((size_t)tiles * 8);
  v.rcnt = (int32_t*)take((size_t)tiles * 4);
  v.base = (int64_t*)take((size_t)tiles * 8);
  v.blist = (int32_t*)take((size_t)tiles * 4);
  v.bsum = (int64_t*)take((size_t)(tiles / FK_T + 1) * 8);
  v.cx = (int64_t*)take((size_t)tiles * 5 * 8);
  // a tile holds at most FT_LMAX frames
  v.fblk = (int32_t*)take((size_t)(tiles * (FT_LMAX / FR_T) + 1) * 4);
  v.total = o;
  return v;
}

// fs_link's grid: the check's workgroups (the last to finish goes on).
constexpr unsigned FL_BLOCKS = 16;

// The smallest plausible frame body of the tile map's nodes (the smallest
// ZooKeeper body is 8 bytes: a ping's xid + type).  A real frame that short
// is still framed exactly (the map sends its chain to the serial walk).
constexpr int32_t FS_MINB = 8;

// fs_tile's tiles (waves) per block: four 12 KiB slices, 3 blocks a CU (as
// many waves as two-slice blocks, half the workgroups to dispatch: GET 0.585
// -> 0.581 ms, mix and watch -0.7 %, profiles/r5_fs_tpb_ab.log)
constexpr int FS_TPB = 4;

// One fs_tile launch over the workspace: window W (256 .. 2048), G tiles a
// wave.  tile_launch (frame_tile.hip) holds the single-tile instances (G ==
// 1; lng: long-frame mode), group256_launch / group512_launch
// (frame_group256.hip, frame_group512.hip) the groups of that window (G = 2 /
// 4 / 8).  tflags: fs_tile's test bits (zk_frame_scan's flags).
struct TileLaunch {
  const uint8_t* buf;
  const int64_t* n_dev;
  int64_t n_cap, maxp;
  const FsWs* ws;
  int64_t* dbg;
  int32_t tflags;
  int W, G;
  bool lng;
};
int tile_launch(const TileLaunch& l, hipStream_t st);
int group256_launch(const TileLaunch& l, hipStream_t st);
int group512_launch(const TileLaunch& l, hipStream_t st);

// fs_link over the workspace (frame_link.hip); ldbg: its debug rows or null.
int link_launch(const uint8_t* buf, const int64_t* n_dev, int64_t n_cap,
                int64_t maxp, const FsWs& ws, int64_t cap, int64_t* result,
                int64_t* ldbg, hipStream_t st);

}  // namespace zk
