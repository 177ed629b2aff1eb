// The rule of SET_ACL (csrc/kernels/zk_setacl.h setacl_frame, setacl_admin,
// setacl_verdict) on the host, a stand-alone program for ASan + UBSan
// (tests/test_setacl_host.py):
//   setacl_host <file>
// <file>: any number of cases, each four little-endian int64 words kind, a, b,
// n and then n bytes.  Every frame, vector and record block sits in a heap
// block of exactly its length, so a read past one is a sanitizer report.
// Prints one line a case:
//   kind 0  setacl_frame(the bytes, base = a, L = n - a):
//           "status xid pl version poff voff vlen" (offsets relative to base;
//           -1 none)
//   kind 1  the whole rule for one frame: setacl_frame, then setacl_admin on
//           the node's current ACL when it is asked for, then setacl_verdict:
//           the error code.  The bytes: le32 exists, check, kind (SA_*), addr,
//           aversion, nids (-1: no identity table), per identity le32 length
//           and the id, le32 length of the node's current vector and the
//           vector, then the frame.  The identities go into records of a
//           block of exactly nids * AUTH_REC bytes, the vector and the frame
//           into blocks of their own.
//   kind 2  front_walk_setacl over the bytes as one segment (quota = a,
//           max_packet = b): "take nfr flag"
//   kind 3  front_walk_ordered_setacl (quota = a, max_packet = b >> 1,
//           has_acl = b & 1): "take nfr flag nwr"
//   kind 4  mix_class_setacl(the bytes as one frame body, has_acl = a) and
//           mix_class beside it: "class class"
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels
//        tools/setacl_host.cpp -o setacl_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_front.h"
#include "zk_setacl.h"

static uint8_t* block(const uint8_t* src, int64_t n) {
  // (malloc(0) may return null; a block of one byte is never read)
  uint8_t* p = (uint8_t*)std::malloc(n > 0 ? (size_t)n : 1);
  if (n > 0) std::memcpy(p, src, (size_t)n);
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
    int64_t h[4];
    std::memcpy(h, raw.data() + o, 32);
    o += 32;
    const int64_t kind = h[0], a = h[1], b = h[2], n = h[3];
    if (n < 0 || n > (1 << 26) || o + (size_t)n > raw.size()) return 1;
    const uint8_t* in = raw.data() + o;
    o += (size_t)n;
    int rc = 0;
    switch (kind) {
      case 0: {
        if (a < 0 || a > n) { rc = 1; break; }
        uint8_t* p = block(in, n);
        const zk::SetAclFrame fr = zk::setacl_frame(p, a, n - a);
        std::printf("%d %d %d %d %lld %lld %lld\n", (int)fr.status,
                    (int)fr.xid, (int)fr.pl, (int)fr.version,
                    (long long)(fr.poff < 0 ? -1 : fr.poff - a),
                    (long long)(fr.voff < 0 ? -1 : fr.voff - a),
                    (long long)fr.vlen);
        std::free(p);
        break;
      }
      case 1: {
        if (n < 24) { rc = 1; break; }
        int32_t w[6];
        std::memcpy(w, in, 24);
        const int32_t exists = w[0], check = w[1], akind = w[2], addr = w[3],
                      aversion = w[4], nids = w[5];
        if (nids < -1 || nids > zk::AUTH_K) { rc = 1; break; }
        uint8_t* recs = nids < 0 ? nullptr : (uint8_t*)std::calloc(
            nids > 0 ? (size_t)nids * zk::AUTH_REC : 1, 1);
        int64_t k = 24;
        for (int32_t r = 0; r < nids && rc == 0; ++r) {
          int32_t il;
          if (k + 4 > n) { rc = 1; break; }
          std::memcpy(&il, in + k, 4);
          k += 4;
          const int32_t nb = il < 0 ? 0 : il;
          if (nb > zk::AUTH_ID_MAX || k + nb > n) { rc = 1; break; }
          std::memcpy(recs + (size_t)r * zk::AUTH_REC, &il, 4);
          std::memcpy(recs + (size_t)r * zk::AUTH_REC + 4, in + k, (size_t)nb);
          k += nb;
        }
        int32_t vl = 0;
        if (rc == 0 && k + 4 <= n) {
          std::memcpy(&vl, in + k, 4);
          k += 4;
        } else {
          rc = 1;
        }
        if (rc == 0 && (vl < 0 || k + vl > n)) rc = 1;
        if (rc == 0) {
          uint8_t* vec = block(in + k, vl);
          k += vl;
          uint8_t* fr = block(in + k, n - k);
          const zk::SetAclFrame sf = zk::setacl_frame(fr, 0, n - k);
          const bool admin = check == 0 ||
              zk::setacl_admin(akind, vec, vl, (uint32_t)addr, recs, nids);
          std::printf("%d\n", (int)zk::setacl_verdict(
                                  sf.status, exists != 0, admin, sf.version,
                                  aversion));
          std::free(fr);
          std::free(vec);
        }
        std::free(recs);
        break;
      }
      case 2: {
        uint8_t* p = block(in, n);
        const zk::FrontCut c = zk::front_walk_setacl(
            n, a, b, [&](int64_t q) { return zk::ld_be32(p + q); });
        std::printf("%lld %d %d\n", (long long)c.take, c.nfr, c.flag);
        std::free(p);
        break;
      }
      case 3: {
        uint8_t* p = block(in, n);
        const zk::FrontCutOrd c = zk::front_walk_ordered_setacl(
            n, a, b >> 1, (b & 1) != 0,
            [&](int64_t q) { return zk::ld_be32(p + q); });
        std::printf("%lld %d %d %d\n", (long long)c.take, c.nfr, c.flag,
                    c.nwr);
        std::free(p);
        break;
      }
      case 4: {
        uint8_t* p = block(in, n);
        std::printf("%d %d\n", (int)zk::mix_class_setacl(p, 0, n, a != 0),
                    (int)zk::mix_class(p, 0, n, a != 0));
        std::free(p);
        break;
      }
      default:
        rc = 1;
    }
    if (rc != 0) return rc;
  }
  return o == raw.size() ? 0 : 1;
}
