// K1 — parallel length-prefixed frame scan: the entry points, the plan and
// the small kernels (fs_rows, fs_small).  The design note and what the K1
// files share: zk_frame_scan.h; the tile pass: zk_frame_tile.h, frame_tile.hip,
// frame_group256.hip, frame_group512.hip; the link pass: frame_link.hip.
#include "zk_frame_scan.h"

namespace zk {

// (body offset, length) rows: one wave per tile, 4 tiles per block.  A
// stale tile (its exact entry, exit and count looked up by fs_link's chase)
// has no recorded frame starts for that entry: its wave stages the tile in
// LDS and walks them first.
__global__ __launch_bounds__(256) void fs_rows(
    const uint8_t* __restrict__ buf, const int64_t* __restrict__ n_dev,
    int64_t n_cap, const uint16_t* __restrict__ list,
    const uint16_t* __restrict__ pre, const int64_t* __restrict__ rec_meta,
    const int64_t* __restrict__ rec_entry,
    const int64_t* __restrict__ rec_exit,
    const int64_t* __restrict__ base, const int64_t* __restrict__ bsum,
    const int64_t* __restrict__ lastk, int64_t* __restrict__ foff,
    int32_t* __restrict__ flen, int64_t cap, uint64_t* __restrict__ lbw,
    uint64_t* __restrict__ lbw_tail) {
  // (only the staged tile: 16 KiB a block keeps fs_rows at full occupancy;
  // a frame-start array beside it cost the var-size GET 3x in fs_rows)
  __shared__ __attribute__((aligned(16))) uint8_t stage[4][FT_STAGE];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t t = (int64_t)blockIdx.x * 4 + wv;
  const int64_t n = stream_len(n_dev, n_cap);
  if (t == 0) {
    // fs_link's minima and broken-link count, for the next scan; and its
    // barrier words (the big repair): every fs_link workgroup has ended
    // (stream order), so a late one of an abandoned barrier can no longer
    // leave an arrival or the abort flag to the next scan
    if (lane == 0) {
      lbw_tail[LW_MINS] = 0;
      lbw_tail[LW_MINS + 1] = 0;
      lbw_tail[LW_NOSPEC] = 0;
      lbw_tail[LW_GRID + FL_NB] = 0;
    }
    if (lane < LW_END - LW_BIG) lbw_tail[LW_BIG + lane] = 0;
  }
  if (t * FT_S >= n) return;
  // the scan is over for this tile: clear its candidate flags, so the next
  // scan of this workspace needs no memset (zk_frame_scan clean=1)
  if (lane == 0) {
    lbw[2 * t] = 0;
    lbw[2 * t + 1] = 0;
  }
  if (t > *lastk) return;
  const int64_t b = bsum[t / FK_T] + base[t];
  const int64_t m = rec_meta[t];
  const int64_t x = rec_exit[t];
  const int32_t cnt = m_cnt(m);
  auto row = [&](int32_t k, int64_t p, int64_t q) {
    const int64_t idx = b + k;
    if (idx < cap) {
      foff[idx] = p + 4;
      flen[idx] = (int32_t)(q - p - 4);
    }
  };
  if (m_stale(m)) {
    const int32_t c = __builtin_amdgcn_readfirstlane(
        (int32_t)(rec_entry[t] - t * FT_S));
    fr_walk_stale<false>(buf, n, t, c, cnt, x, stage[wv], lane, row);
    return;
  }
  // lengths come from the recorded starts, no stream read (zk_frame_rows.h)
  for (int32_t k = lane; k < cnt; k += 64) {
    int64_t p, q;
    fr_bounds(list, pre, t, m, x, k, p, q);
    row(k, p, q);
  }
}

// A stream of one tile at most (handshakes, a SET_WATCHES frame, small
// batches): staged once and walked frame by frame by one wave — one launch
// instead of fs_tile, fs_link and fs_rows (the storm's two handshake
// streams a step were six launches).  Same results as the tiled scan.
__global__ __launch_bounds__(64) void fs_small(
    const uint8_t* __restrict__ buf, const int64_t* __restrict__ n_dev,
    int64_t n_cap, int64_t maxp, int64_t* __restrict__ foff,
    int32_t* __restrict__ flen, int64_t cap, int64_t* __restrict__ result) {
  __shared__ __attribute__((aligned(16))) uint8_t sb[FT_STAGE];
  const int lane = threadIdx.x;
  const int64_t n = stream_len(n_dev, n_cap);       // (<= FT_S)
  fc_stage<FT_S>(buf, n, 0, sb, lane);
  int32_t c = 0, k = 0;
  bool bad = false;
  const int32_t n32 = (int32_t)n;
  while (c + 4 <= n32) {
    const int32_t len = __builtin_amdgcn_readfirstlane(lds_be32(sb, c));
    if (len < 0 || (int64_t)len > maxp) { bad = true; break; }
    if (c + 4 + len > n32) break;                   // the carry
    if (lane == 0 && k < cap) {
      foff[k] = c + 4;
      flen[k] = len;
    }
    ++k;
    c += 4 + len;
  }
  if (lane == 0) {
    result[0] = k;
    result[1] = c;
    result[2] = bad ? 1 : 0;
    result[3] = k > cap ? 1 : 0;
  }
}

// scan flag: frames may be longer than the window (fs_tile's frontier
// passes past the window, and survivor exits past it as candidates)
constexpr int32_t FS_LONG = 2;
// scan flag: rows deferred — no fs_rows launch; a consumer that reads the
// tile lists (zk_frame_tiles, zk_frame_rows.h) writes the rows and clears
// the flags.  Not for streams of one tile at most (fs_small has no lists).
constexpr int32_t FS_DEFER = 1 << 24;

// `window` values with this bit: FS_LONG (zkmi.ops.batch.frame_window sets
// it when the window is below the stream's largest frame)
constexpr int32_t FS_WIN_LONG = 1 << 16;

static int fs_window(int32_t window) {
  window &= FS_WIN_LONG - 1;
  return window <= 256 ? 256 : window <= 512 ? 512
       : window <= 1024 ? 1024 : 2048;
}

// ZKMI_FS_DBG=1: fs_tile writes per-tile timestamps (start, survivor done,
// entry known, walk done), the walked prefix and the survivor's frame count
// into a debug buffer (zk_frame_scan_dbg copies it out).  Diagnostics only.
static int64_t* g_dbg = nullptr;
static int64_t g_dbg_tiles = 0;
static int64_t* fs_dbg_buf(int64_t tiles) {
  static int on = -1;
  if (on < 0) on = getenv("ZKMI_FS_DBG") != nullptr;
  if (!on) return nullptr;
  if (tiles > g_dbg_tiles) {
    if (g_dbg) (void)hipFree(g_dbg);
    // a row per tile (fs_tile) + fs_link's: its phase clock, every block's
    // entry / check-done clocks, the common path's ticket / end clocks
    if (hipMalloc(&g_dbg, (tiles + FL_DBG_ROWS) * 8 * 8) != hipSuccess)
      return nullptr;
    (void)hipMemset(g_dbg, 0, (tiles + FL_DBG_ROWS) * 8 * 8);
    g_dbg_tiles = tiles;
  }
  return g_dbg;
}

}  // namespace zk

extern "C" {

int64_t zk_frame_scan_workspace(int64_t n) {
  return (int64_t)zk::fs_view(nullptr, n).total;
}

// K1 over buf[0, n) with n = min(*n_dev, n_cap) read ON THE DEVICE (n_dev
// null: n = n_cap): fs_tile, fs_link, fs_rows (after one memset of the
// tiles' flags).  The grids cover n_cap and tiles past n return at once, so
// a producer's device byte count (an encoder's `total`) is scanned with no
// host read and no byte past it is touched.  The launches depend only on
// n_cap, so a scan can be captured in a HIP graph and replayed over any
// length up to it.
//
// result (device int64[4]): [0] frames found, [1] stop offset (consumed
// bytes; start of the carry or of the bad frame), [2] 1 if the stop is a
// BAD_LENGTH frame, [3] 1 if the frame table overflowed `cap` (rows past
// cap are dropped).
//
// `window` (256 / 512 / 1024 / 2048 bytes) is the speculative entry window
// per 4 KiB tile: a chain can only enter a tile inside it when frames are
// <= window bytes.  Longer frames stay exact (fs_link re-walks the tiles
// after them from the exact exit, one tile at a time), so the window is a
// performance hint: the smallest one covering the stream's usual frame
// size makes the scan cheapest.  maxp must be <= 16 MiB (the protocol's
// frame limit).
// clean != 0: the workspace's flags were left cleared by the previous scan
// of it over the same n_cap (fs_rows / fs_link clear what they used), so
// the memset is skipped.  A stale flag could only cost speed, never
// correctness (fs_tile / fs_link check every speculated entry).
// flags: bit 1 (FS_LONG) frames may be longer than the window (a window
// below the stream's largest frame: fs_tile's frontier passes); tests of
// the link repair: bit 0 no speculated tile entries; bits 8..23 P > 0:
// every P-th tile (t % P == 1) takes a garbage entry.
int zk_frame_scan(const uint8_t* buf, const int64_t* n_dev, int64_t n_cap,
                  int64_t maxp, uint8_t* ws, int64_t ws_bytes, int64_t* foff,
                  int32_t* flen, int64_t cap, int64_t* result, int32_t window,
                  int32_t clean, int32_t flags, hipStream_t st) {
  using namespace zk;
  const int W = fs_window(window);
  const bool defer = (flags & FS_DEFER) != 0;
  flags &= ~FS_DEFER;
  if (window & FS_WIN_LONG) flags |= FS_LONG;
  if (maxp > FC_MAXP || maxp < 0) return -3;
  const FsWs v = fs_view(ws, n_cap);
  if ((int64_t)v.total > ws_bytes) return -1;
  const int64_t tiles = v.tiles;
  // (no tile lists a consumer could take for a stream of one tile at most:
  // zk_frame_tiles refuses it, whichever path the scan itself would take)
  if (defer && n_cap <= FT_S) return -5;
  if (n_cap <= FT_S && !(flags & (1 | 0xFFFF00)) &&
      fs_dbg_buf(tiles) == nullptr) {
    fs_small<<<1, 64, 0, st>>>(buf, n_dev, n_cap, maxp, foff, flen, cap,
                               result);
    ZK_LAUNCH_CHECK();
    return 0;
  }
  // X flags, the stats, the check's minima and fs_link's grid words start
  // at zero
  if (!clean && hipMemsetAsync(v.lbw, 0, v.lbw_bytes, st) != hipSuccess)
    return -4;
  int64_t* dbg = fs_dbg_buf(tiles);
  // tiles a wave: groups (the map once, the chain walked on) for streams
  // of large frames within a small window; long-frame streams take single
  // tiles (the link repair's test flags apply to a group's first tile)
  int G = ((flags >> 4) & 15) + 1;
  if ((flags & FS_LONG) || W > 512) G = 1;
  G = G >= 8 ? 8 : G >= 4 ? 4 : G >= 2 ? 2 : 1;
  const TileLaunch tl{buf, n_dev, n_cap, maxp, &v, dbg, flags, W, G,
                      (flags & FS_LONG) != 0};
  int rc = G == 1 ? tile_launch(tl, st)
           : W == 256 ? group256_launch(tl, st) : group512_launch(tl, st);
  if (rc) return rc;
  rc = link_launch(buf, n_dev, n_cap, maxp, v, cap, result,
                   dbg ? dbg + 8 * tiles : nullptr, st);
  if (rc || defer) return rc;
  fs_rows<<<(unsigned)((tiles + 3) / 4), 256, 0, st>>>(
      buf, n_dev, n_cap, v.list, v.pre, v.rmeta, v.rent, v.rexit, v.base,
      v.bsum, &v.tail->lastk, foff, flen, cap, v.lbw, (uint64_t*)v.tail);
  ZK_LAUNCH_CHECK();
  return 0;
}

// The tile lists of a (rows-deferred) scan over n_cap bytes on workspace ws,
// for the consumers' launchers.
int zk_frame_tiles(const uint8_t* buf, const int64_t* n_dev, int64_t n_cap,
                   uint8_t* ws, int64_t ws_bytes, ZkFrameTiles* out) {
  using namespace zk;
  if (n_cap <= FT_S) return -2;
  const FsWs v = fs_view(ws, n_cap);
  if ((int64_t)v.total > ws_bytes) return -1;
  out->buf = buf;
  out->n_dev = n_dev;
  out->n_cap = n_cap;
  out->list = v.list;
  out->pre = v.pre;
  out->rec_meta = v.rmeta;
  out->rec_entry = v.rent;
  out->rec_exit = v.rexit;
  out->base = v.base;
  out->bsum = v.bsum;
  out->lastk = &v.tail->lastk;
  out->fblk = v.fblk;
  out->lbw = v.lbw;
  out->tiles = v.tiles;
  return 0;
}

// Chain statistics of the last scan of workspace `ws` over a buffer of
// n_cap bytes, into out4 (host): tiles without a speculated entry, tiles
// re-walked, repair rounds, tiles a chase looked up.
int zk_frame_scan_stats(const uint8_t* ws, int64_t n_cap, uint32_t* out4,
                        hipStream_t st) {
  using namespace zk;
  FsTail* t = fs_view(const_cast<uint8_t*>(ws), n_cap).tail;
  const uint64_t* word[4] = {&t->nospec_total, &t->walked, &t->rounds,
                             &t->looked};
  for (int k = 0; k < 4; ++k)
    if (hipMemcpyAsync(out4 + k, word[k], 4, hipMemcpyDeviceToHost, st) !=
        hipSuccess)
      return -1;
  if (hipStreamSynchronize(st) != hipSuccess) return -1;
  // counters since the last read (scans of a clean workspace skip the
  // memset that used to reset them)
  if (hipMemsetAsync(t, 0, offsetof(FsTail, mins), st) != hipSuccess)
    return -1;
  return hipStreamSynchronize(st) == hipSuccess ? 0 : -1;
}

// rows = tiles + FL_DBG_ROWS: past the tiles' rows, fs_link's phase clock of
// a chase repair (start, chases done, barrier, links checked, end; [6] / [7]
// the exact chase's start and end), then every block's entry and check-done
// clocks (4 rows), then the common path's bases start / end ([0] / [1])
int zk_frame_scan_dbg(int64_t* host, int64_t tiles) {
  if (!zk::g_dbg || tiles > zk::g_dbg_tiles + zk::FL_DBG_ROWS) return -1;
  return hipMemcpy(host, zk::g_dbg, tiles * 8 * 8, hipMemcpyDeviceToHost) ==
                 hipSuccess ? 0 : -1;
}

}  // extern "C"
