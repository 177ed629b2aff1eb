// The rules of the ordered front end on the host — csrc/kernels/zk_front.h
// front_walk_ordered (the cut's ordered rule) and csrc/kernels/zk_order_clip.h
// clip_overflow / clip_deferred / clip_range (deferral in the ordered session
// serve), the text front.hip and tree_order.hip run — a stand-alone program
// for ASan + UBSan (tests/test_order_clip_host.py):
//   order_clip_host <file>
// <file>: any number of cases, each eight little-endian int64 words h[0..7],
// h[0] the kind, then the kind's tables.  Every table and every segment sits
// in a heap block of exactly its length, so a read past one is a sanitizer
// report.
//   kind 0  an ordered walk: h[1] = len, h[2] = quota, h[3] = max_packet,
//           h[4] = has_acl; the len bytes of one segment.  Prints
//           "take nfr flag nwr".
//   kind 1  the clip: h[1] = ncap, h[2] = S, h[3] = passes, h[4] = nfr (the
//           batch's frames, <= ncap); rank[ncap] (uint8), cls[ncap], sub[ncap],
//           f_seg[ncap] (int32).  clipf[s] is the smallest i < nfr with a
//           segment in [0, S) that clip_overflow holds for (ncap: none).
//           Prints clipf[S], then clip_deferred of the nfr frames, on one line.
//   kind 2  the ranges: h[1] = S, h[2] = ncap, h[3] = nfr; clipf[S],
//           rep_off[S + 1], rec_off[ncap], off[ncap], starts[S + 1] (int64).
//           Prints "rep_end used" of every segment, on one line.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/order_clip_host.cpp -o order_clip_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_front.h"
#include "zk_order_clip.h"

template <typename T>
static T* block(const uint8_t* src, int64_t n) {
  // (malloc(0) may return null; a block of one byte is never read)
  T* p = (T*)std::malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && src != nullptr) std::memcpy(p, src, (size_t)n * sizeof(T));
  return p;
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
      uint8_t* b = block<uint8_t>(in.data() + o, len);
      o += (size_t)len;
      const zk::FrontCutOrd c = zk::front_walk_ordered(
          len, h[2], h[3], h[4] != 0,
          [&](int64_t p) { return zk::ld_be32(b + p); });
      std::free(b);
      std::printf("%lld %d %d %d\n", (long long)c.take, c.nfr, c.flag, c.nwr);
    } else if (h[0] == 1) {
      const int64_t ncap = h[1], S = h[2], nfr = h[4];
      const int32_t passes = (int32_t)h[3];
      if (ncap < 1 || ncap > lim || S < 1 || S > lim || nfr < 0 ||
          nfr > ncap || o + (size_t)ncap * 13 > in.size())
        return 1;
      uint8_t* rank = block<uint8_t>(in.data() + o, ncap);
      o += (size_t)ncap;
      int32_t* cls = block<int32_t>(in.data() + o, ncap);
      o += (size_t)ncap * 4;
      int32_t* sub = block<int32_t>(in.data() + o, ncap);
      o += (size_t)ncap * 4;
      int32_t* f_seg = block<int32_t>(in.data() + o, ncap);
      o += (size_t)ncap * 4;
      int64_t* clipf = block<int64_t>(nullptr, S);
      for (int64_t s = 0; s < S; ++s) clipf[s] = ncap;
      for (int64_t i = 0; i < nfr; ++i) {
        const int64_t sg = f_seg[i];
        if (sg >= 0 && sg < S &&
            zk::clip_overflow(cls[i], sub[i], rank, ncap, passes) &&
            i < clipf[sg])
          clipf[sg] = i;
      }
      for (int64_t s = 0; s < S; ++s)
        std::printf(s ? " %lld" : "%lld", (long long)clipf[s]);
      for (int64_t i = 0; i < nfr; ++i)
        std::printf(" %d", zk::clip_deferred(clipf, S, f_seg[i], i) ? 1 : 0);
      std::printf("\n");
      std::free(rank);
      std::free(cls);
      std::free(sub);
      std::free(f_seg);
      std::free(clipf);
    } else if (h[0] == 2) {
      const int64_t S = h[1], ncap = h[2], nfr = h[3];
      if (S < 1 || S > lim || ncap < 0 || ncap > lim || nfr < 0 ||
          nfr > ncap || o + (size_t)(3 * S + 2 + 2 * ncap) * 8 > in.size())
        return 1;
      int64_t* clipf = block<int64_t>(in.data() + o, S);
      o += (size_t)S * 8;
      int64_t* rep_off = block<int64_t>(in.data() + o, S + 1);
      o += (size_t)(S + 1) * 8;
      int64_t* rec_off = block<int64_t>(in.data() + o, ncap);
      o += (size_t)ncap * 8;
      int64_t* off = block<int64_t>(in.data() + o, ncap);
      o += (size_t)ncap * 8;
      int64_t* starts = block<int64_t>(in.data() + o, S + 1);
      o += (size_t)(S + 1) * 8;
      for (int64_t s = 0; s < S; ++s) {
        const zk::ClipRange r =
            zk::clip_range(clipf, rep_off, rec_off, off, starts, nfr, s);
        std::printf(s ? " %lld %lld" : "%lld %lld", (long long)r.rep_end,
                    (long long)r.used);
      }
      std::printf("\n");
      std::free(clipf);
      std::free(rep_off);
      std::free(rec_off);
      std::free(off);
      std::free(starts);
    } else {
      return 1;
    }
  }
  return o == in.size() ? 0 : 1;
}
