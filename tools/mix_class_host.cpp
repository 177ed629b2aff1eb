// The mixed-batch class function (csrc/kernels/zk_mix.h mix_class — the text
// the split kernel runs) on the host, a stand-alone program for ASan + UBSan
// (tests/test_mix_host.py):
//   mix_class_host <file> <has_acl 0|1>
// <file>: frames as on the wire (a big-endian length word, then the body).
// Each body is classified in a heap block of exactly its length, so a read
// past the frame is a sanitizer report; prints one class per line.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/mix_class_host.cpp -o mix_class_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_mix.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <file> <has_acl 0|1>\n", argv[0]);
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
  const bool has_acl = std::atoi(argv[2]) != 0;
  size_t o = 0;
  while (o + 4 <= raw.size()) {
    const int32_t len = zk::ld_be32(raw.data() + o);
    if (len < 0 || o + 4 + (size_t)len > raw.size()) {
      std::fprintf(stderr, "bad length word at %zu\n", o);
      return 1;
    }
    // (malloc(0) may return null; a block of one byte is never read)
    uint8_t* body = (uint8_t*)std::malloc(len > 0 ? (size_t)len : 1);
    if (len > 0) std::memcpy(body, raw.data() + o + 4, (size_t)len);
    std::printf("%d\n", (int)zk::mix_class(body, 0, len, has_acl));
    std::free(body);
    o += 4 + (size_t)len;
  }
  return o == raw.size() ? 0 : 1;
}
