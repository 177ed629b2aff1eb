// The session batches' segment rule (csrc/kernels/zk_sess.h — the text the
// kernels of csrc/kernels/tree_sess.hip run) on the host, a stand-alone
// program for ASan + UBSan (tests/test_sess_host.py):
//   sess_host <file>
// <file>: any number of cases, each two little-endian int64 words S and nf,
// then starts[S + 1] (int64), off[nf] (int64) and len[nf] (int32).  Every
// table sits in a heap block of exactly its length, so a read past it is a
// sanitizer report.  Prints three lines a case: f_seg[nf], first[S + 1], and
// bad with the first bad segment (-1: none).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/sess_host.cpp -o sess_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_sess.h"

template <typename T>
static T* block(const uint8_t* src, int64_t n) {
  // (malloc(0) may return null; a block of one byte is never read)
  T* p = (T*)std::malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0) std::memcpy(p, src, (size_t)n * sizeof(T));
  return p;
}

// --self N SEED: N random sound tables (boundaries on frame boundaries, empty
// segments among them), each in exact heap blocks; every frame must lie in
// its segment, nothing torn, first[S] the frame count.
static int self_test(long n, unsigned long long seed) {
  auto rnd = [&](int64_t m) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return (int64_t)((seed >> 33) % (unsigned long long)m);
  };
  for (long k = 0; k < n; ++k) {
    const int64_t nf = rnd(50), S = 1 + rnd(70);
    std::vector<int64_t> b(1, 0), off_v, st(S + 1, 0);
    std::vector<int32_t> len_v;
    for (int64_t j = 0; j < nf; ++j) {
      const int32_t l = (int32_t)rnd(64);
      off_v.push_back(b.back() + 4);
      len_v.push_back(l);
      b.push_back(b.back() + 4 + l);
    }
    int64_t at = 0;                        // boundary index, non-decreasing
    for (int64_t s = 1; s < S; ++s) {
      at += rnd(3) == 0 ? rnd(nf - at + 1) : 0;
      st[s] = b[at];
    }
    st[S] = b.back();
    int64_t* starts = block<int64_t>((const uint8_t*)st.data(), S + 1);
    int64_t* off = block<int64_t>((const uint8_t*)off_v.data(), nf);
    int32_t* len = block<int32_t>((const uint8_t*)len_v.data(), nf);
    int bad = 0;
    for (int64_t j = 0; j < nf; ++j) {
      const int64_t seg = zk::sess_seg(starts, S, off[j] - 4);
      if (zk::sess_torn(starts, S, seg, off[j] + len[j])) ++bad;
      else if (starts[seg] > off[j] - 4) ++bad;
    }
    for (int64_t s = 0; s <= S; ++s) {
      bad += zk::sess_boundary_bad(starts, S, s);
      const int64_t fi = zk::sess_first(off, nf, starts[s]);
      if (fi < 0 || fi > nf || (s == S && fi != nf)) ++bad;
    }
    std::free(starts);
    std::free(off);
    std::free(len);
    if (bad) {
      std::fprintf(stderr, "self test: table %ld is not sound\n", k);
      return 1;
    }
  }
  std::printf("sess_host: %ld sound tables\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::strcmp(argv[1], "--self") == 0)
    return self_test(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <file> | --self N SEED\n", argv[0]);
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
  while (o + 16 <= raw.size()) {
    int64_t S, nf;
    std::memcpy(&S, raw.data() + o, 8);
    std::memcpy(&nf, raw.data() + o + 8, 8);
    o += 16;
    if (S < 1 || nf < 0 || S > (1 << 24) || nf > (1 << 24)) return 1;
    const size_t need = (size_t)(S + 1) * 8 + (size_t)nf * 12;
    if (o + need > raw.size()) return 1;
    int64_t* starts = block<int64_t>(raw.data() + o, S + 1);
    o += (size_t)(S + 1) * 8;
    int64_t* off = block<int64_t>(raw.data() + o, nf);
    o += (size_t)nf * 8;
    int32_t* len = block<int32_t>(raw.data() + o, nf);
    o += (size_t)nf * 4;
    int64_t bad = 0, first_bad = -1;
    auto mark = [&](int64_t s) {
      if (first_bad < 0 || s < first_bad) first_bad = s;
    };
    for (int64_t j = 0; j < nf; ++j) {
      const int64_t seg = zk::sess_seg(starts, S, off[j] - 4);
      if (zk::sess_torn(starts, S, seg, off[j] + len[j])) {
        ++bad;
        mark(seg < 0 ? 0 : seg);
      }
      std::printf(j ? " %lld" : "%lld", (long long)seg);
    }
    std::printf("\n");
    for (int64_t s = 0; s <= S; ++s) {
      const int32_t b = zk::sess_boundary_bad(starts, S, s);
      if (b) {
        bad += b;
        mark(s);
      }
      std::printf(s ? " %lld" : "%lld",
                  (long long)zk::sess_first(off, nf, starts[s]));
    }
    std::printf("\n%lld %lld\n", (long long)bad, (long long)first_bad);
    std::free(starts);
    std::free(off);
    std::free(len);
  }
  return o == raw.size() ? 0 : 1;
}
