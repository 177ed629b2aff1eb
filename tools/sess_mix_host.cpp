// The rules of a session batch of any op mix (csrc/kernels/zk_sess.h
// sess_refusal, sess_split_at, sess_xid — the text the session instances of
// tree_list.hip / tree_acl.hip and sess_split_seg_k of tree_sess.hip run) on
// the host, a stand-alone program for ASan + UBSan
// (tests/test_sess_mix_host.py):
//   sess_mix_host <file>
// <file>: any number of cases, each four little-endian int64 words S, n, ncap
// and bad, then seg_state[S], f_seg[n], cls[n], sub[n] (int32 each) and n
// frames' first 8 body bytes with their int32 body length in front
// (12 bytes a frame).  Every table sits in a heap block of exactly its
// length, so a read or a write past it is a sanitizer report.  Prints three
// lines a case: the refusal of every frame, its xid as a refused frame's
// reply carries it, and the three class tables f_seg_c[3][ncap] laid end to
// end after a scalar walk of the split-segments rule over frames
// [0, min(n, ncap)) (-7: not written).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/sess_mix_host.cpp -o sess_mix_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_sess.h"

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
  while (o + 32 <= raw.size()) {
    int64_t S, n, ncap, badw;
    std::memcpy(&S, raw.data() + o, 8);
    std::memcpy(&n, raw.data() + o + 8, 8);
    std::memcpy(&ncap, raw.data() + o + 16, 8);
    std::memcpy(&badw, raw.data() + o + 24, 8);
    o += 32;
    if (S < 1 || n < 0 || ncap < 0 || S > (1 << 24) || n > (1 << 24) ||
        ncap > (1 << 24))
      return 1;
    const size_t need = (size_t)S * 4 + (size_t)n * (12 + 12);
    if (o + need > raw.size()) return 1;
    int32_t* seg_state = block<int32_t>(raw.data() + o, S);
    o += (size_t)S * 4;
    int32_t* f_seg = block<int32_t>(raw.data() + o, n);
    o += (size_t)n * 4;
    int32_t* cls = block<int32_t>(raw.data() + o, n);
    o += (size_t)n * 4;
    int32_t* sub = block<int32_t>(raw.data() + o, n);
    o += (size_t)n * 4;
    int64_t* bad = block<int64_t>((const uint8_t*)&badw, 1);
    // -- the refusal of every frame
    for (int64_t i = 0; i < n; ++i)
      std::printf(i ? " %d" : "%d",
                  (int)zk::sess_refusal(bad, seg_state, S, f_seg[i]));
    std::printf("\n");
    // -- a refused frame's xid: the body alone in a block of its length
    for (int64_t i = 0; i < n; ++i) {
      int32_t L;
      std::memcpy(&L, raw.data() + o, 4);
      if (L < 0 || L > 8) return 1;
      uint8_t* body = block<uint8_t>(raw.data() + o + 4, L);
      std::printf(i ? " %d" : "%d", (int)zk::sess_xid(body, 0, L));
      std::free(body);
      o += 12;
    }
    std::printf("\n");
    // -- the split-segments rule, a scalar walk of the kernel's lanes
    int32_t* tab = block<int32_t>(nullptr, 3 * ncap);
    for (int64_t k = 0; k < 3 * ncap; ++k) tab[k] = -7;
    const int64_t nf = n < ncap ? n : ncap;
    for (int64_t i = 0; i < nf; ++i) {
      const int64_t at = zk::sess_split_at(cls[i], sub[i], ncap);
      if (at >= 0) tab[at] = f_seg[i];
    }
    for (int64_t k = 0; k < 3 * ncap; ++k)
      std::printf(k ? " %d" : "%d", (int)tab[k]);
    std::printf("\n");
    std::free(seg_state);
    std::free(f_seg);
    std::free(cls);
    std::free(sub);
    std::free(bad);
    std::free(tab);
  }
  return o == raw.size() ? 0 : 1;
}
