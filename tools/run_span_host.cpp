// K1's run gather on the host — csrc/kernels/zk_run_span.h run_want /
// run_word_in / run_accept / run_tiles_covered / run_tile, the text
// zk_frame_tile.h ft_gather_issue and ft_gather_take run — a stand-alone
// program for ASan + UBSan (tests/test_run_span_host.py):
//   run_span_host <S> [<S> ...]
// For every frame size S, every entry offset 0..255 into the tile the run
// enters, every group of G = 2, 4, 8, 16 tiles (the run enters the group's
// second tile, so G - 1 tiles are left) and stream ends in every one of those
// tiles (at a frame's end, inside a header, inside a body, at the tile's
// end), a stream of back-to-back S-byte frames sits in a heap block of
// EXACTLY the stream's length.  The gather is played as the wave's lanes
// play it, round after round of 256 frames: a word is read only where
// run_word_in allows (a read outside the stream is a sanitizer report), the
// leading accepted frames are the round's run, and the tiles it covers whole
// (run_tile) are compared with a byte-by-byte walk of the same bytes: each
// tile's first frame, frame count, entry and exit, and that the gather stops
// exactly at the tile the walk cannot leave.  Prints "<S> <cases>" a size;
// exits 1 on a mismatch.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/run_span_host.cpp -o run_span_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_run_span.h"

namespace {

constexpr int32_t CAP = 256;             // frames a gather round asks for
constexpr int32_t MAXP = 1 << 20;

int32_t be32(const uint8_t* p) {
  return (int32_t)((uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 |
                   (uint32_t)p[2] << 8 | (uint32_t)p[3]);
}

struct Tile {
  int32_t first, count, entry, exit;     // exit < 0: the walk ends inside
};

// The hop-by-hop walk from crel over buf[0, nrel): per tile (0 = the one
// crel lies in) its frames; a tile the chain cannot leave has exit -1.
std::vector<Tile> walk(const uint8_t* buf, int32_t nrel, int32_t crel,
                       int tiles) {
  std::vector<Tile> out;
  int32_t c = crel, idx = 0;
  for (int q = 0; q < tiles; ++q) {
    Tile t{idx, 0, c, -1};
    const int32_t tend = (q + 1) * zk::RUN_TILE;
    for (;;) {
      if (c >= tend) { t.exit = c; break; }
      if (c + 4 > nrel) break;
      const int32_t len = be32(buf + c);
      if (len < 0 || len > MAXP || c + 4 + len > nrel) break;
      c += 4 + len;
      ++t.count;
      ++idx;
    }
    out.push_back(t);
    if (t.exit < 0) break;
  }
  return out;
}

int fail(const char* what, int32_t S, int off, int G, int32_t n, int q) {
  std::fprintf(stderr, "S %d entry %d G %d n %d tile %d: %s\n", S, off, G, n,
               q, what);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <S> [<S> ...]\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; ++a) {
    const int32_t S = std::atoi(argv[a]);
    if (S < 16 || S > zk::RUN_TILE) return 2;
    long cases = 0;
    for (int G : {2, 4, 8, 16})
      for (int off = 0; off < 256; ++off) {
        const int tiles = G - 1;
        const int32_t full = tiles * zk::RUN_TILE + 2 * S;
        for (int et = 0; et < tiles; ++et) {
          // stream ends in tile et: at the end of the last frame that ends
          // in it (fe), 2 bytes and S / 2 bytes into that frame (it is cut:
          // in its header, in its body), at the tile's end, past the group
          const int32_t in_tile = ((et + 1) * zk::RUN_TILE - off) / S;
          const int32_t fe = off + in_tile * S;
          const int32_t ends[] = {fe, fe - S + 2, fe - S / 2,
                                  (et + 1) * zk::RUN_TILE, full};
          for (int32_t n : ends) {
            if (n <= off || n > full) continue;
            uint8_t* buf = (uint8_t*)std::malloc((size_t)n);
            for (int32_t k = 0; k < n; ++k) buf[k] = (uint8_t)(k * 37 + 11);
            for (int32_t p = off; p < n; p += S) {
              const uint8_t h[4] = {0, 0, (uint8_t)((S - 4) >> 8),
                                    (uint8_t)(S - 4)};
              for (int k = 0; k < 4 && p + k < n; ++k) buf[p + k] = h[k];
            }
            const std::vector<Tile> ref = walk(buf, n, off, tiles);
            // the gather, round after round (ft_group_tail's loop)
            int32_t c = off, idx = 0;
            int q0 = 0;
            bool more = true;
            while (more && q0 < tiles) {
              const int32_t crel = c - q0 * zk::RUN_TILE;
              if (crel < 0 || crel >= zk::RUN_TILE) break;
              const uint8_t* tb = buf + (size_t)q0 * zk::RUN_TILE;
              const int32_t nrel = n - q0 * zk::RUN_TILE;
              const int32_t room = tiles - q0;
              const int32_t want =
                  zk::run_want(crel, S, room * zk::RUN_TILE, CAP);
              int32_t acc = 0;
              for (int32_t j = 0; j < want; ++j) {
                const int32_t p = crel + j * S;
                if (!zk::run_word_in(p, nrel)) break;
                uint32_t w;
                std::memcpy(&w, tb + p, 4);          // the lane's load
                const int32_t len = (int32_t)__builtin_bswap32(w);
                if (!zk::run_accept(len, S, p, nrel, MAXP)) break;
                ++acc;
              }
              more = acc == CAP;
              int32_t cov = zk::run_tiles_covered(crel, S, acc);
              if (cov > room) cov = room;
              if (cov == 0) break;
              for (int q = 0; q < cov; ++q) {
                const zk::RunTile r = zk::run_tile(crel, S, acc, q);
                if ((size_t)(q0 + q) >= ref.size())
                  return fail("tile past the walk", S, off, G, n, q0 + q);
                const Tile& t = ref[(size_t)(q0 + q)];
                if (t.exit < 0)
                  return fail("covered a tile the walk ends in", S, off, G,
                              n, q0 + q);
                if (idx + r.first != t.first || r.count != t.count ||
                    q0 * zk::RUN_TILE + r.entry != t.entry ||
                    q0 * zk::RUN_TILE + r.exit != t.exit)
                  return fail("record differs", S, off, G, n, q0 + q);
                // every frame of the tile lands inside its list
                for (int32_t j = r.first; j < r.first + r.count; ++j)
                  if ((crel + j * S) / zk::RUN_TILE != q)
                    return fail("frame in another tile", S, off, G, n,
                                q0 + q);
              }
              const zk::RunTile l = zk::run_tile(crel, S, acc, cov - 1);
              idx += l.first + l.count;
              c = q0 * zk::RUN_TILE + l.exit;
              q0 += cov;
            }
            // the gather stopped at the tile the walk cannot leave, or took
            // the whole group
            const int done = q0;
            int leave = 0;
            while ((size_t)leave < ref.size() && ref[(size_t)leave].exit >= 0)
              ++leave;
            if (done != leave)
              return fail("tiles covered differ from the walk's", S, off, G,
                          n, done);
            std::free(buf);
            ++cases;
          }
        }
      }
    std::printf("%d %ld\n", S, cases);
  }
  return 0;
}
