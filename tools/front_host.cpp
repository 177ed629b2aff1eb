// The rules of the front end's I/O staging (csrc/kernels/zk_front.h
// front_walk / front_is_write, front_boundary_bad, front_piece_at,
// front_owner_scan / front_piece — the text front.hip runs) on the host, a
// stand-alone program for ASan + UBSan (tests/test_front_host.py):
//   front_host <file>
// <file>: any number of cases, each eight little-endian int64 words h[0..7],
// h[0] the kind, then the kind's tables.  Every table and every segment sits
// in a heap block of exactly its length, so a read past one is a sanitizer
// report.
//   kind 0  a walk: h[1] = len, h[2] = quota, h[3] = max_packet; the len bytes
//           of one segment.  Prints "take nfr flag".
//   kind 1  a cut: h[1] = S, h[2] = n, h[3] = quota, h[4] = max_packet;
//           raw_starts[S + 1] (int64), raw[n].  Prints the table-fault word,
//           then "take nfr flag" of every segment, on one line (a faulted
//           table takes nothing; a sound one walks each segment from a block
//           of its own).
//   kind 2  pieces: h[1] = S, h[2] = which tables are there (bit 0 rep_off,
//           bits 1..3 the three slot_off, bit 4 err), h[3] = err, h[4..7] =
//           the four streams' bytes; rep_off[S + 1] (int64) when there,
//           wslots[S] (int32), each slot_off[65] (int64) that is there.
//           Prints the count of segments on a slot another one owns, then
//           "stream src len" of the 4 S pieces, on one line.
//   kind 3  front_piece_at: h[1] = P, h[2] = nq; off[P] (int64), nq
//           destination bytes (int64).  Prints the nq pieces.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/front_host.cpp -o front_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_front.h"

template <typename T>
static T* block(const uint8_t* src, int64_t n) {
  // (malloc(0) may return null; a block of one byte is never read)
  T* p = (T*)std::malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && src != nullptr) std::memcpy(p, src, (size_t)n * sizeof(T));
  return p;
}

static zk::FrontCut walk(const uint8_t* seg, int64_t len, int64_t quota,
                         int64_t max_packet) {
  uint8_t* b = block<uint8_t>(seg, len);
  const zk::FrontCut c = zk::front_walk(
      len, quota, max_packet, [&](int64_t p) { return zk::ld_be32(b + p); });
  std::free(b);
  return c;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <file>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> in;
  uint8_t chunk[4096];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0)
    in.insert(in.end(), chunk, chunk + got);
  std::fclose(f);
  const int64_t lim = 1 << 24;
  size_t o = 0;
  while (o + 64 <= in.size()) {
    int64_t h[8];
    std::memcpy(h, in.data() + o, 64);
    o += 64;
    if (h[0] == 0) {
      const int64_t len = h[1];
      if (len < 0 || len > lim || o + (size_t)len > in.size()) return 1;
      const zk::FrontCut c = walk(in.data() + o, len, h[2], h[3]);
      o += (size_t)len;
      std::printf("%lld %d %d\n", (long long)c.take, c.nfr, c.flag);
    } else if (h[0] == 1) {
      const int64_t S = h[1], n = h[2];
      if (S < 1 || S > lim || n < 0 || n > lim ||
          o + (size_t)(S + 1) * 8 + (size_t)n > in.size())
        return 1;
      int64_t* starts = block<int64_t>(in.data() + o, S + 1);
      o += (size_t)(S + 1) * 8;
      const uint8_t* raw = in.data() + o;
      o += (size_t)n;
      int64_t fault = 0;
      for (int64_t s = 0; s <= S; ++s)
        if (zk::front_boundary_bad(starts, S, n, s) != 0) fault = 1;
      std::printf("%lld", (long long)fault);
      for (int64_t s = 0; s < S; ++s) {
        zk::FrontCut c{0, 0, 0};
        if (fault == 0)
          c = walk(raw + starts[s], starts[s + 1] - starts[s], h[3], h[4]);
        std::printf(" %lld %d %d", (long long)c.take, c.nfr, c.flag);
      }
      std::printf("\n");
      std::free(starts);
    } else if (h[0] == 2) {
      const int64_t S = h[1], have = h[2];
      if (S < 1 || S > lim) return 1;
      size_t need = (size_t)S * 4;
      if (have & 1) need += (size_t)(S + 1) * 8;
      for (int k = 0; k < 3; ++k)
        if (have & (2 << k)) need += 65 * 8;
      if (o + need > in.size()) return 1;
      zk::FrontTx t;
      int64_t* rep = nullptr;
      if (have & 1) {
        rep = block<int64_t>(in.data() + o, S + 1);
        o += (size_t)(S + 1) * 8;
      }
      int32_t* wslots = block<int32_t>(in.data() + o, S);
      o += (size_t)S * 4;
      int64_t* so[3] = {nullptr, nullptr, nullptr};
      for (int k = 0; k < 3; ++k)
        if (have & (2 << k)) {
          so[k] = block<int64_t>(in.data() + o, 65);
          o += 65 * 8;
        }
      int32_t* err = nullptr;
      if (have & 16) {
        const int32_t e = (int32_t)h[3];
        err = block<int32_t>((const uint8_t*)&e, 1);
      }
      int64_t* owner = block<int64_t>(nullptr, zk::FRONT_SLOTS);
      int64_t dup = 0;
      for (int32_t w = 0; w < zk::FRONT_SLOTS; ++w) {
        int64_t own = -1, named = 0;
        zk::front_owner_scan(wslots, S, 0, w, own, named);
        owner[w] = own;
        if (named > 1) dup += named - 1;
      }
      t.rep_off = rep;
      for (int k = 0; k < 3; ++k) t.slot_off[k] = so[k];
      for (int k = 0; k < 4; ++k) t.cap[k] = h[4 + k];
      t.err = err;
      t.wslots = wslots;
      t.owner = owner;
      t.S = S;
      std::printf("%lld", (long long)dup);
      for (int64_t s = 0; s < S; ++s)
        for (int32_t k = 0; k < zk::FRONT_PIECES; ++k) {
          const zk::FrontPiece p = zk::front_piece(t, s, k);
          std::printf(" %d %lld %lld", p.stream, (long long)p.src,
                      (long long)p.len);
        }
      std::printf("\n");
      std::free(rep);
      std::free(wslots);
      for (int k = 0; k < 3; ++k) std::free(so[k]);
      std::free(err);
      std::free(owner);
    } else if (h[0] == 3) {
      const int64_t P = h[1], nq = h[2];
      if (P < 1 || P > lim || nq < 0 || nq > lim ||
          o + (size_t)(P + nq) * 8 > in.size())
        return 1;
      int64_t* off = block<int64_t>(in.data() + o, P);
      o += (size_t)P * 8;
      int64_t* q = block<int64_t>(in.data() + o, nq);
      o += (size_t)nq * 8;
      for (int64_t k = 0; k < nq; ++k)
        std::printf(k ? " %lld" : "%lld",
                    (long long)zk::front_piece_at(off, P, q[k]));
      std::printf("\n");
      std::free(off);
      std::free(q);
    } else {
      return 1;
    }
  }
  return o == in.size() ? 0 : 1;
}
