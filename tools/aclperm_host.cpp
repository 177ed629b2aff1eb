// The rule of ACL enforcement (csrc/kernels/zk_aclperm.h aclperm_need,
// aclperm_ip_match, aclperm_permits, aclperm_parent_cut — the text
// tree_aclperm.hip runs) on the host, a stand-alone program for ASan + UBSan
// (tests/test_aclperm_host.py):
//   aclperm_host <file>
// <file>: any number of cases, each four little-endian int64 words kind, a, b,
// n and then n bytes.  The bytes sit in a heap block of exactly n bytes, so a
// read past them is a sanitizer report.  Prints one line a case:
//   kind 0  aclperm_need(op = a): "perm target"
//   kind 1  aclperm_ip_match(the bytes as the id, addr = a): 0 / 1
//   kind 2  aclperm_permits(the bytes as the vector, perm = a, addr = b): 0 / 1
//   kind 3  aclperm_parent_cut(the bytes as the path): the cut
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/aclperm_host.cpp -o aclperm_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_aclperm.h"

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
    int64_t h[4];
    std::memcpy(h, raw.data() + o, 32);
    o += 32;
    const int64_t kind = h[0], a = h[1], b = h[2], n = h[3];
    if (n < 0 || n > (1 << 24) || o + (size_t)n > raw.size()) return 1;
    // (malloc(0) may return null; a block of one byte is never read)
    uint8_t* p = (uint8_t*)std::malloc(n > 0 ? (size_t)n : 1);
    if (n > 0) std::memcpy(p, raw.data() + o, (size_t)n);
    o += (size_t)n;
    switch (kind) {
      case 0: {
        const zk::AclNeed need = zk::aclperm_need((int32_t)a);
        std::printf("%d %d\n", (int)need.perm, (int)need.target);
        break;
      }
      case 1:
        std::printf("%d\n", zk::aclperm_ip_match(p, n, (uint32_t)a) ? 1 : 0);
        break;
      case 2:
        std::printf("%d\n", zk::aclperm_permits(p, n, (int32_t)a,
                                                (uint32_t)b) ? 1 : 0);
        break;
      case 3:
        std::printf("%d\n", (int)zk::aclperm_parent_cut(p, (int32_t)n));
        break;
      default:
        std::free(p);
        return 1;
    }
    std::free(p);
  }
  return o == raw.size() ? 0 : 1;
}
