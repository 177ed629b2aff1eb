// The rule of AUTH with digest identities (csrc/kernels/zk_auth.h auth_frame,
// auth_sha1, auth_b64, auth_identity, auth_match, aclperm_permits_auth — the
// text tree_auth.hip runs) on the host, a stand-alone program for ASan + UBSan
// (tests/test_auth_host.py):
//   auth_host <file>
// <file>: any number of cases, each four little-endian int64 words kind, a, b,
// n and then n bytes.  The bytes sit in a heap block of exactly n bytes (kind
// 5: two blocks), so a read past them is a sanitizer report.  Prints one line
// a case:
//   kind 0  auth_frame(the bytes, base = a, L = n - a): "status xid type n off"
//           (off relative to base; -1 none)
//   kind 1  auth_sha1(the bytes): 40 hex digits
//   kind 2  auth_b64(the 20 bytes): the 28 characters
//   kind 3  auth_identity(the bytes): the identity in hex
//   kind 4  aclperm_permits(the bytes as the vector, perm = a, addr = b): 0 / 1
//   kind 5  aclperm_permits_auth(perm = a, addr = b): 0 / 1.  The bytes: le32
//           nids, per identity le32 length and the id, then the vector.  The
//           identities go into records of a block of exactly nids * AUTH_REC
//           bytes, the vector into a block of its own.
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels
//        tools/auth_host.cpp -o auth_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_auth.h"

static void hex(const uint8_t* p, int n) {
  for (int k = 0; k < n; ++k) std::printf("%02x", p[k]);
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
    int rc = 0;
    switch (kind) {
      case 0: {
        if (a < 0 || a > n) { rc = 1; break; }
        const zk::AuthFrame fr = zk::auth_frame(p, a, n - a);
        std::printf("%d %d %d %d %lld\n", (int)fr.status, (int)fr.xid,
                    (int)fr.type, (int)fr.n,
                    (long long)(fr.off < 0 ? -1 : fr.off - a));
        break;
      }
      case 1: {
        if (n > zk::AUTH_MAX) { rc = 1; break; }
        uint8_t out[20];
        zk::auth_sha1(p, (int32_t)n, out);
        hex(out, 20);
        break;
      }
      case 2: {
        if (n != 20) { rc = 1; break; }
        uint8_t* out = (uint8_t*)std::malloc(zk::AUTH_B64);
        zk::auth_b64(p, out);
        std::printf("%.28s\n", (const char*)out);
        std::free(out);
        break;
      }
      case 3: {
        if (n > zk::AUTH_MAX) { rc = 1; break; }
        uint8_t* id = (uint8_t*)std::malloc(zk::AUTH_ID_MAX);
        int32_t il = -1;
        zk::auth_identity(p, (int32_t)n, id, il);
        if (il < 0 || il > zk::AUTH_ID_MAX) rc = 1; else hex(id, il);
        std::free(id);
        break;
      }
      case 4:
        std::printf("%d\n", zk::aclperm_permits(p, n, (int32_t)a,
                                                (uint32_t)b) ? 1 : 0);
        break;
      case 5: {
        if (n < 4) { rc = 1; break; }
        int32_t nids;
        std::memcpy(&nids, p, 4);
        if (nids < 0 || nids > zk::AUTH_K) { rc = 1; break; }
        uint8_t* recs = (uint8_t*)std::calloc(
            nids > 0 ? (size_t)nids * zk::AUTH_REC : 1, 1);
        int64_t k = 4;
        for (int32_t r = 0; r < nids && rc == 0; ++r) {
          int32_t il;
          if (k + 4 > n) { rc = 1; break; }
          std::memcpy(&il, p + k, 4);
          k += 4;
          // (a record may carry a length no identity has: auth_match's guard)
          const int32_t nb = il < 0 ? 0 : il;
          if (nb > zk::AUTH_ID_MAX || k + nb > n) { rc = 1; break; }
          std::memcpy(recs + (size_t)r * zk::AUTH_REC, &il, 4);
          std::memcpy(recs + (size_t)r * zk::AUTH_REC + 4, p + k, (size_t)nb);
          k += nb;
        }
        if (rc == 0) {
          const int64_t vl = n - k;
          uint8_t* vec = (uint8_t*)std::malloc(vl > 0 ? (size_t)vl : 1);
          if (vl > 0) std::memcpy(vec, p + k, (size_t)vl);
          std::printf("%d\n", zk::aclperm_permits_auth(
                                  vec, vl, (int32_t)a, (uint32_t)b, recs,
                                  nids) ? 1 : 0);
          std::free(vec);
        }
        std::free(recs);
        break;
      }
      default:
        rc = 1;
    }
    std::free(p);
    if (rc != 0) return rc;
  }
  return o == raw.size() ? 0 : 1;
}
