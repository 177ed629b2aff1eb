// The arithmetic of K1's run gather (zk_frame_tile.h ft_gather_issue, ft_gather_take) in plain
// C++: no HIP include, so the host compiler builds the very text the kernel
// runs (tools/run_span_host.cpp puts it under ASan + UBSan on a machine
// without a GPU).
//
// A RUN is `count` frames of S bytes each lying back to back from stream
// offset c: frame j starts at c + j * S, its big-endian length word reads
// S - 4.  The gather reads the words where the frames of a run WOULD start
// and accepts the leading ones that repeat the length; by induction that
// prefix is what a hop-by-hop walk finds.  The tiles (RUN_TILE bytes each)
// the accepted run covers whole — the run has a frame that ends at or past
// the tile's end — get their records from the arithmetic below; the tile the
// run ends in is walked.
#pragma once
#include <stdint.h>

#include "zk_wire.h"   // ZK_HD

namespace zk {

constexpr int32_t RUN_TILE = 4096;

// Positions are relative to the start of the tile the run enters (crel, the
// run's first frame, lies in it) and the stream ends at nrel; a gather
// round spans at most a few hundred frames of at most RUN_TILE bytes, so
// they are 32-bit.

// May the 4-byte word at position p of the stream be loaded?
ZK_HD bool run_word_in(int32_t p, int32_t nrel) {
  return p >= 0 && p + 4 <= nrel;
}

// Is the frame at p whose length word reads `len` the run's next frame: the
// run's length, the frame inside the stream, the length legal (the hop's
// test)?
ZK_HD bool run_accept(int32_t len, int32_t S, int32_t p, int32_t nrel,
                      int32_t maxp) {
  return len == S - 4 && p + S <= nrel && (uint32_t)len <= (uint32_t)maxp;
}

// Frames the gather asks for from crel: those starting before the group's
// end gerel (> crel; both relative to the start of c's tile), at most `cap`.
ZK_HD int32_t run_want(int32_t crel, int32_t S, int32_t gerel, int32_t cap) {
  const int32_t w = (gerel - crel + S - 1) / S;
  return w < cap ? w : cap;
}

// Frames of the run that start before offset x (relative to c: x - c may be
// negative), clipped to [0, count].
ZK_HD int32_t run_frames_before(int32_t S, int32_t count, int32_t xrel) {
  if (xrel <= 0) return 0;
  const int32_t k = (xrel + S - 1) / S;
  return k < count ? k : count;
}

// Tiles from the one c lies in that the run of `count` frames covers whole.
// crel: c relative to that tile's start (0 <= crel < RUN_TILE).
ZK_HD int32_t run_tiles_covered(int32_t crel, int32_t S, int32_t count) {
  return (int32_t)(((int64_t)crel + (int64_t)count * S) / RUN_TILE);
}

// Tile q (0 = the tile c lies in, q < run_tiles_covered) of the run: the
// index of its first frame, its frames, its entry and its exit (the end of
// its last frame: at or past the tile's end), both relative to the start of
// tile 0.
struct RunTile {
  int32_t first, count;
  int32_t entry, exit;
};
ZK_HD RunTile run_tile(int32_t crel, int32_t S, int32_t count, int32_t q) {
  RunTile r;
  r.first = run_frames_before(S, count, q * RUN_TILE - crel);
  const int32_t next = run_frames_before(S, count, (q + 1) * RUN_TILE - crel);
  r.count = next - r.first;
  r.entry = crel + r.first * S;
  r.exit = crel + next * S;
  return r;
}

}  // namespace zk
