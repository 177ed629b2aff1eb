// The rules of a session batch's SET_WATCHES catch-up (csrc/kernels/
// zk_resume.h resume_frame, resume_walk, resume_decide, resume_entry_frame —
// the text tree_resume.hip runs) on the host, a stand-alone program for
// ASan + UBSan (tests/test_resume_host.py):
//   resume_host <file>
// <file>: any number of cases, each eight little-endian int64 words S, seg,
// bad, L, piece, nd, nb, nq, then seg_state[S] and wslots[S] (int32 each), the
// L bytes of one frame body, nd decisions of five int64 words (kind, there,
// mzxid, pzxid, rel), base[nb] and nq entry indices (int64 each).  Every table
// and the frame sit in heap blocks of exactly their length, so a read past
// one is a sanitizer report.  Prints six lines a case:
//   resume_frame's verdict for the frame (rx = the body alone, offset 0)
//   the walk over the whole frame: ok, the count, then kind:offset:length
//   the walk fed `piece` bytes at a time (the kernel's chunks): the same
//   parse_request's status, opcode and path count of the body
//   resume_decide of every decision
//   resume_entry_frame of every index over base
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/resume_host.cpp -o resume_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_resume.h"

template <typename T>
static T* block(const uint8_t* src, int64_t n) {
  // (malloc(0) may return null; a block of one byte is never read)
  T* p = (T*)std::malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && src != nullptr) std::memcpy(p, src, (size_t)n * sizeof(T));
  return p;
}

static void walk(const uint8_t* body, int64_t L, int64_t piece) {
  std::vector<int64_t> out;
  zk::ResumeWalk w = zk::resume_walk_begin(0);
  auto rd = [&](int64_t k) -> int32_t {
    // (the walk's promise: only whole words of the frame, from the lists on)
    if (k < zk::RS_HEAD || k + 4 > L) std::abort();
    return zk::ld_be32(body + k);
  };
  auto emit = [&](int64_t m, int32_t g, int64_t po, int32_t pl) {
    if (m != (int64_t)out.size() / 3) std::abort();
    out.push_back(g);
    out.push_back(po);
    out.push_back(pl);
  };
  int64_t avail = 0;
  // (a frame shorter than its head still gets one call: done, nothing read)
  do {
    avail = piece > 0 && avail + piece < L ? avail + piece : L;
    zk::resume_walk(w, avail, L, rd, emit);
  } while (!w.done && avail < L);
  if (!w.done) std::abort();          // the whole frame was fed
  if (w.m != (int64_t)out.size() / 3) std::abort();
  std::printf("%d %lld", w.ok ? 1 : 0, (long long)w.m);
  for (size_t i = 0; i < out.size(); i += 3)
    std::printf(" %lld:%lld:%lld", (long long)out[i], (long long)out[i + 1],
                (long long)out[i + 2]);
  std::printf("\n");
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
  std::vector<uint8_t> raw;
  uint8_t chunk[4096];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0)
    raw.insert(raw.end(), chunk, chunk + got);
  std::fclose(f);
  size_t o = 0;
  while (o + 64 <= raw.size()) {
    int64_t h[8];
    std::memcpy(h, raw.data() + o, 64);
    o += 64;
    const int64_t S = h[0], seg = h[1], L = h[3], piece = h[4], nd = h[5],
                  nb = h[6], nq = h[7];
    const int64_t lim = 1 << 24;
    if (S < 1 || S > lim || L < 0 || L > lim || piece < 0 || nd < 0 ||
        nd > lim || nb < 0 || nb > lim || nq < 0 || nq > lim)
      return 1;
    const size_t need = (size_t)S * 8 + (size_t)L + (size_t)nd * 40 +
                        (size_t)nb * 8 + (size_t)nq * 8;
    if (o + need > raw.size()) return 1;
    int64_t* bad = block<int64_t>((const uint8_t*)&h[2], 1);
    int32_t* seg_state = block<int32_t>(raw.data() + o, S);
    o += (size_t)S * 4;
    int32_t* wslots = block<int32_t>(raw.data() + o, S);
    o += (size_t)S * 4;
    uint8_t* body = block<uint8_t>(raw.data() + o, L);
    o += (size_t)L;
    std::printf("%d\n", (int)zk::resume_frame(body, L, 0, L, bad, seg_state,
                                              wslots, S, seg));
    walk(body, L, 0);
    walk(body, L, piece);
    const zk::ReqFields rq = zk::parse_request(body, 0, L);
    std::printf("%d %d %d\n", (int)rq.status, (int)rq.op, (int)rq.vc);
    for (int64_t i = 0; i < nd; ++i) {
      int64_t d[5];
      std::memcpy(d, raw.data() + o, 40);
      o += 40;
      std::printf(i ? " %d" : "%d",
                  (int)zk::resume_decide((int32_t)d[0], d[1] != 0, d[2], d[3],
                                         d[4]));
    }
    std::printf("\n");
    int64_t* base = block<int64_t>(raw.data() + o, nb);
    o += (size_t)nb * 8;
    for (int64_t i = 0; i < nq; ++i) {
      int64_t e;
      std::memcpy(&e, raw.data() + o, 8);
      o += 8;
      std::printf(i ? " %lld" : "%lld",
                  (long long)zk::resume_entry_frame(base, nb, e));
    }
    std::printf("\n");
    std::free(bad);
    std::free(seg_state);
    std::free(wslots);
    std::free(body);
    std::free(base);
  }
  return o == raw.size() ? 0 : 1;
}
