// The device request parser (csrc/kernels/zk_wire.h: parse_request,
// skip_strings, skip_acl — the text tree_serve_k, decode_requests_k and
// list_mark_k run) as a host program, for AddressSanitizer + UBSan:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -fno-sanitize-recover=all -Icsrc/kernels tools/fuzz_reqparse.cpp
//
//   fuzz_reqparse --fuzz N SEED    N generated and mutated request bodies,
//       each copied into a heap block of exactly its length (a read one
//       byte past the frame is an ASan report); every (offset, length) the
//       parser returns must lie inside the body, every skip_* result within
//       the bytes it was given.  Exit 0, or 1 with the failing body in hex.
//   fuzz_reqparse --corpus FILE    FILE holds bodies, each after its length
//       as a big-endian int32 (a framed stream); one line a body:
//       status xid op arg path_off path_len data_off data_len vec_count
//       rel_zxid (offsets from the body's start, -1 none).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zk_wire.h"

namespace {

typedef std::vector<uint8_t> Bytes;

struct Rng {
  uint64_t s;
  uint64_t next() {                       // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
  bool chance(uint32_t pct) { return below(100) < pct; }
};

void put32(Bytes& b, int32_t v) {
  for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t)((uint32_t)v >> s));
}
void put64(Bytes& b, int64_t v) {
  for (int s = 56; s >= 0; s -= 8) b.push_back((uint8_t)((uint64_t)v >> s));
}
// a Jute buffer: empty goes out as length -1 (lib/jute-buffer.js:127-130)
void put_buf(Bytes& b, Rng& r, uint32_t maxlen) {
  const uint32_t n = r.chance(20) ? 0 : r.below(maxlen + 1);
  if (n == 0) { put32(b, r.chance(50) ? -1 : 0); return; }
  put32(b, (int32_t)n);
  for (uint32_t i = 0; i < n; ++i) b.push_back((uint8_t)r.below(0x80));
}
void put_acl(Bytes& b, Rng& r) {
  const uint32_t n = r.below(3);
  put32(b, (int32_t)n);
  for (uint32_t i = 0; i < n; ++i) {
    put32(b, (int32_t)r.below(32));
    put_buf(b, r, 8);
    put_buf(b, r, 12);
  }
}
void put_strings(Bytes& b, Rng& r) {
  const uint32_t n = r.below(4);
  put32(b, (int32_t)n);
  for (uint32_t i = 0; i < n; ++i) put_buf(b, r, 24);
}

const int32_t OPS[] = {zk::OP_GET_DATA, zk::OP_EXISTS, zk::OP_GET_CHILDREN,
                       zk::OP_GET_CHILDREN2, zk::OP_CREATE, zk::OP_DELETE,
                       zk::OP_SET_DATA, zk::OP_GET_ACL, zk::OP_SYNC,
                       zk::OP_SET_WATCHES, zk::OP_PING, zk::OP_CLOSE_SESSION};
const int32_t BAD_OPS[] = {7, 13, 14, 100, 9999, 0, -1, 102, -10};
const int32_t WORDS[] = {-1, INT32_MIN, 0, 1, 3, 5, 17, 67, 68, 69, 0x7f, 0x100,
                         0x7f7f, 0x10000, 0x7f000000, 0x7ffffffb, 0x7ffffffc,
                         0x7fffffff};

Bytes gen_request(Rng& r) {
  Bytes b;
  const int32_t op = OPS[r.below(sizeof OPS / sizeof OPS[0])];
  put32(b, (int32_t)r.next());
  put32(b, op);
  switch (op) {
    case zk::OP_GET_DATA: case zk::OP_EXISTS: case zk::OP_GET_CHILDREN:
    case zk::OP_GET_CHILDREN2:
      put_buf(b, r, 40);
      b.push_back((uint8_t)r.below(2));
      break;
    case zk::OP_CREATE:
      put_buf(b, r, 40); put_buf(b, r, 64); put_acl(b, r);
      put32(b, (int32_t)r.below(4));
      break;
    case zk::OP_DELETE:
      put_buf(b, r, 40); put32(b, (int32_t)r.below(12) - 1);
      break;
    case zk::OP_SET_DATA:
      put_buf(b, r, 40); put_buf(b, r, 64); put32(b, (int32_t)r.below(12) - 1);
      break;
    case zk::OP_GET_ACL: case zk::OP_SYNC:
      put_buf(b, r, 40);
      break;
    case zk::OP_SET_WATCHES:
      put64(b, (int64_t)r.next());
      put_strings(b, r); put_strings(b, r); put_strings(b, r);
      break;
    default:
      break;
  }
  return b;
}

void mutate(Bytes& b, Rng& r) {
  switch (r.below(8)) {
    case 0: case 1:                       // as generated
      break;
    case 2: case 3:                       // one word overwritten, anywhere
      if (b.size() >= 4) {
        const size_t at = r.below((uint32_t)(b.size() - 3));
        const int32_t v = WORDS[r.below(sizeof WORDS / sizeof WORDS[0])];
        for (int k = 0; k < 4; ++k)
          b[at + k] = (uint8_t)((uint32_t)v >> (24 - 8 * k));
      }
      break;
    case 4:                               // cut short (0 .. size - 1)
      b.resize(r.below((uint32_t)b.size()));
      break;
    case 5: {                             // trailing bytes
      const uint32_t n = 1 + r.below(80);
      for (uint32_t i = 0; i < n; ++i) b.push_back((uint8_t)r.next());
      break;
    }
    case 6: {                             // another opcode over the same body
      const int32_t op = r.chance(50)
          ? BAD_OPS[r.below(sizeof BAD_OPS / sizeof BAD_OPS[0])]
          : OPS[r.below(sizeof OPS / sizeof OPS[0])];
      for (int k = 0; k < 4; ++k)
        b[4 + k] = (uint8_t)((uint32_t)op >> (24 - 8 * k));
      break;
    }
    default:                              // one random byte
      if (!b.empty()) b[r.below((uint32_t)b.size())] = (uint8_t)r.next();
  }
}

// The body in a heap block of exactly its length.
struct Exact {
  uint8_t* p;
  int64_t n;
  explicit Exact(const Bytes& b) : p(new uint8_t[b.size()]), n((int64_t)b.size()) {
    if (n) memcpy(p, b.data(), b.size());
  }
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

bool inside(int64_t off, int32_t len, int64_t lo, int64_t n) {
  if (off < 0) return off == -1 && len == 0;
  return len >= 0 && off >= lo && off + (int64_t)len <= n;
}

const char* check(const zk::ReqFields& f, int64_t n) {
  if (f.status != zk::ST_OK && f.status != zk::ST_BAD_DECODE &&
      f.status != zk::ST_BAD_OPCODE) return "status";
  if ((n < 8) != (f.status == zk::ST_BAD_DECODE && f.op == zk::OP_UNKNOWN))
    return "short body";
  if (!inside(f.poff, f.pl, 12, n)) return "path outside the body";
  if (!inside(f.doff, f.dl, 16, n)) return "data outside the body";
  if (f.voff < -1 || f.voff > n) return "vector outside the body";
  // (a rejected CREATE keeps the count word it could not walk)
  if (f.vc < 0 || (f.status == zk::ST_OK && (int64_t)f.vc * 4 > n))
    return "vector count";
  if (f.status == zk::ST_OK && f.vc > 0 && f.voff < 0) return "vector offset";
  return nullptr;
}

void dump(const Bytes& b) {
  for (size_t i = 0; i < b.size(); ++i) fprintf(stderr, "%02x", b[i]);
  fprintf(stderr, "\n");
}

int fuzz(long n, uint64_t seed) {
  Rng r{seed};
  long ok = 0, bad = 0, badop = 0;
  for (long it = 0; it < n; ++it) {
    Bytes b = gen_request(r);
    mutate(b, r);
    Exact e(b);
    const zk::ReqFields f = zk::parse_request(e.p, 0, e.n);
    const char* why = check(f, e.n);
    if (why) {
      fprintf(stderr, "case %ld: %s\n", it, why);
      dump(b);
      return 1;
    }
    ok += f.status == zk::ST_OK;
    bad += f.status == zk::ST_BAD_DECODE;
    badop += f.status == zk::ST_BAD_OPCODE;
    // the two walkers on their own, from any offset, with any count
    const int64_t at = e.n ? r.below((uint32_t)e.n + 1) : 0;
    const int32_t cnt = r.chance(50) ? (int32_t)r.below(6)
        : WORDS[r.below(sizeof WORDS / sizeof WORDS[0])];
    const int64_t s = zk::skip_strings(e.p + at, e.n - at, cnt);
    const int64_t a = zk::skip_acl(e.p + at, e.n - at, cnt);
    if (s < -1 || s > e.n - at || a < -1 || a > e.n - at ||
        (cnt <= 0 && (s != 0 || a != 0))) {
      fprintf(stderr, "case %ld: skip at %lld count %d -> %lld / %lld of %lld\n",
              it, (long long)at, cnt, (long long)s, (long long)a,
              (long long)(e.n - at));
      dump(b);
      return 1;
    }
  }
  printf("fuzz: %ld bodies, %ld decoded, %ld bad decode, %ld bad opcode\n", n,
         ok, bad, badop);
  // a generator that stopped reaching a class would prove nothing
  if (n >= 1000 && (ok == 0 || bad == 0 || badop == 0)) {
    fprintf(stderr, "a status class was never reached\n");
    return 1;
  }
  return 0;
}

int corpus(const char* path) {
  FILE* fh = fopen(path, "rb");
  if (!fh) { perror(path); return 2; }
  uint8_t h[4];
  while (fread(h, 1, 4, fh) == 4) {
    const int32_t n = zk::ld_be32(h);
    if (n < 0 || n > (1 << 24)) { fprintf(stderr, "bad length %d\n", n); return 2; }
    Bytes b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, fh) != (size_t)n) {
      fprintf(stderr, "short file\n");
      return 2;
    }
    Exact e(b);
    const zk::ReqFields f = zk::parse_request(e.p, 0, e.n);
    const char* why = check(f, e.n);
    if (why) {
      fprintf(stderr, "%s\n", why);
      dump(b);
      return 1;
    }
    printf("%d %d %d %d %lld %d %lld %d %d %lld\n", f.status, f.xid, f.op, f.arg,
           (long long)f.poff, f.pl, (long long)f.doff, f.dl, f.vc,
           (long long)f.rel);
  }
  fclose(fh);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--fuzz"))
    return fuzz(atol(argv[2]), strtoull(argv[3], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "--corpus")) return corpus(argv[2]);
  fprintf(stderr, "usage: %s --fuzz N SEED | --corpus FILE\n", argv[0]);
  return 2;
}
