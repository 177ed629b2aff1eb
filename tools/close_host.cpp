// The rules of closing many sessions in one pass (csrc/kernels/zk_close.h
// close_frame, close_set_insert / close_set_find, close_drop_mask — the text
// tree_close.hip runs) on the host, a stand-alone program for ASan + UBSan
// (tests/test_close_host.py):
//   close_host <file>
// <file>: any number of cases, each eight little-endian int64 words S, seg,
// bad, L, nk, cap, nq, nw, then seg_state[S] (int32), the L bytes of one frame
// body, the list ids[nk] (int64), nq ids to look up (int64) and nw watcher
// slots (int32).  cap 0: the table size is close_set_cap(nk).  Every table,
// the set's key and rank arrays included, and the frame sit in heap blocks of
// exactly their length, so a read past one is a sanitizer report.  Prints
// five lines a case:
//   close_frame's verdict for the frame (rx = the body alone, offset 0)
//   the table size used, then close_set_insert's result for every listed id
//   close_set_find of every listed id
//   close_set_find of every id to look up
//   the OR of close_drop_mask over the watcher slots, in hex
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/close_host.cpp -o close_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_close.h"

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
    const int64_t S = h[0], seg = h[1], L = h[3], nk = h[4], nq = h[6],
                  nw = h[7];
    const int64_t lim = 1 << 24;
    if (S < 1 || S > lim || L < 0 || L > lim || nk < 0 || nk > lim ||
        h[5] < 0 || h[5] > lim || nq < 0 || nq > lim || nw < 0 || nw > lim)
      return 1;
    const int64_t cap = h[5] > 0 ? h[5] : zk::close_set_cap(nk);
    if ((cap & (cap - 1)) != 0) return 1;
    const size_t need = (size_t)S * 4 + (size_t)L + (size_t)nk * 8 +
                        (size_t)nq * 8 + (size_t)nw * 4;
    if (o + need > raw.size()) return 1;
    int64_t* bad = block<int64_t>((const uint8_t*)&h[2], 1);
    int32_t* seg_state = block<int32_t>(raw.data() + o, S);
    o += (size_t)S * 4;
    uint8_t* body = block<uint8_t>(raw.data() + o, L);
    o += (size_t)L;
    int64_t* ids = block<int64_t>(raw.data() + o, nk);
    o += (size_t)nk * 8;
    int64_t* qs = block<int64_t>(raw.data() + o, nq);
    o += (size_t)nq * 8;
    int32_t* wsl = block<int32_t>(raw.data() + o, nw);
    o += (size_t)nw * 4;
    std::printf("%d\n",
                zk::close_frame(body, L, 0, L, bad, seg_state, S, seg) ? 1 : 0);
    // the tables as the launcher fills them: keys 0, ranks a byte fill of 0x7f
    int64_t* key = block<int64_t>(nullptr, cap);
    int32_t* rank = block<int32_t>(nullptr, cap);
    std::memset(key, 0, (size_t)cap * 8);
    std::memset(rank, 0x7f, (size_t)cap * 4);
    std::printf("%lld", (long long)cap);
    for (int64_t k = 0; k < nk; ++k)
      std::printf(" %d", zk::close_set_insert(key, rank, cap, ids[k],
                                              (int32_t)k,
                                              zk::ClosePlainOps{}) ? 1 : 0);
    std::printf("\n");
    for (int64_t k = 0; k < nk; ++k)
      std::printf(k ? " %d" : "%d",
                  (int)zk::close_set_find(key, rank, cap, ids[k]));
    std::printf("\n");
    for (int64_t k = 0; k < nq; ++k)
      std::printf(k ? " %d" : "%d",
                  (int)zk::close_set_find(key, rank, cap, qs[k]));
    std::printf("\n");
    uint64_t mask = 0;
    for (int64_t k = 0; k < nw; ++k) mask |= zk::close_drop_mask(wsl[k]);
    std::printf("%llx\n", (unsigned long long)mask);
    std::free(bad);
    std::free(seg_state);
    std::free(body);
    std::free(ids);
    std::free(qs);
    std::free(wsl);
    std::free(key);
    std::free(rank);
  }
  return o == raw.size() ? 0 : 1;
}
