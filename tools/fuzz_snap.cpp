// The tree image's structural checks (csrc/kernels/zk_snap.h:
// snap_check_header, snap_check_table, snap_check_record — the text the
// load's check kernels run) as a host program, for AddressSanitizer + UBSan:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -fno-sanitize-recover=all -Icsrc/kernels tools/fuzz_snap.cpp
//
//   fuzz_snap --fuzz N SEED    N generated and mutated images, each copied
//       into a heap block of exactly its length (a read one byte past the
//       image is an ASan report); every field offset a sound record reports
//       must lie inside its span.  Exit 0, or 1 with the failing image in hex.
//   fuzz_snap --corpus FILE    FILE holds images, each after its length as a
//       little-endian u64; one line an image: "code index" as the loader
//       reports them through SNAP_BAD_RECORD (0 -1 for an image whose header,
//       table and records are sound).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zk_snap.h"

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
void put_le64(Bytes& b, int64_t v) {
  for (int s = 0; s < 64; s += 8) b.push_back((uint8_t)((uint64_t)v >> s));
}
void set_le64(Bytes& b, size_t at, int64_t v) {
  for (int s = 0; s < 8; ++s) b[at + s] = (uint8_t)((uint64_t)v >> (8 * s));
}
void put_str(Bytes& b, Rng& r, uint32_t maxlen) {
  const uint32_t n = r.below(maxlen + 1);
  put32(b, n == 0 && r.chance(50) ? -1 : (int32_t)n);
  for (uint32_t i = 0; i < n; ++i) b.push_back((uint8_t)(0x61 + r.below(26)));
}

const int64_t WORDS[] = {-1, INT64_MIN, 0, 1, 4, 7, 8, 9, 64, 67, 68, 72,
                         0x7f, 0x100, 0xffff, 0x1000000, 0x7ffffff8,
                         0x7fffffff, 0x80000000ll, 0x100000000ll,
                         0x7ffffffffffffff8ll, INT64_MAX};

Bytes gen_record(Rng& r) {
  Bytes b;
  const uint32_t pl = 2 + r.below(40);
  put32(b, (int32_t)pl);
  b.push_back('/');
  for (uint32_t i = 1; i < pl; ++i)
    b.push_back((uint8_t)(i + 1 < pl && r.chance(10) ? '/' : 0x61 + r.below(26)));
  const uint32_t dl = r.chance(30) ? 0 : r.below(300);
  for (int i = 0; i < zk::SNAP_STAT; ++i) b.push_back((uint8_t)r.below(256));
  const size_t st = b.size() - zk::SNAP_STAT;
  for (int s = 0; s < 4; ++s) b[st + 52 + s] = (uint8_t)(dl >> (24 - 8 * s));
  put32(b, (int32_t)dl);
  for (uint32_t i = 0; i < dl; ++i) b.push_back((uint8_t)r.below(256));
  if (r.chance(10)) {
    put32(b, -1);
  } else {
    const uint32_t n = 1 + r.below(3);
    put32(b, (int32_t)n);
    for (uint32_t i = 0; i < n; ++i) {
      put32(b, (int32_t)r.below(32));
      put_str(b, r, 8);
      put_str(b, r, 12);
    }
  }
  while (b.size() & 7) b.push_back(0);
  return b;
}

Bytes gen_image(Rng& r) {
  const uint32_t n = r.chance(10) ? 0 : 1 + r.below(6);
  std::vector<Bytes> recs;
  int64_t body = 0;
  for (uint32_t i = 0; i < n; ++i) {
    recs.push_back(gen_record(r));
    body += (int64_t)recs.back().size();
  }
  Bytes b;
  put_le64(b, (int64_t)zk::SNAP_MAGIC);
  put_le64(b, zk::SNAP_VERSION);
  put_le64(b, n);
  put_le64(b, body);
  for (int i = 0; i < 4; ++i) put_le64(b, (int64_t)r.next());
  int64_t o = 0;
  put_le64(b, 0);
  for (auto& x : recs) put_le64(b, o += (int64_t)x.size());
  for (auto& x : recs) b.insert(b.end(), x.begin(), x.end());
  return b;
}

void mutate(Bytes& b, Rng& r) {
  const uint32_t k = 1 + r.below(3);
  for (uint32_t j = 0; j < k && !b.empty(); ++j) {
    switch (r.below(6)) {
      case 0: b.resize(r.below((uint32_t)b.size() + 1)); break;
      case 1: b[r.below((uint32_t)b.size())] ^= (uint8_t)(1u << r.below(8)); break;
      case 2: {                         // a header / table word
        const size_t words = b.size() / 8;
        if (words == 0) break;
        const size_t w = r.below((uint32_t)(words < 16 ? words : 16));
        set_le64(b, 8 * w, WORDS[r.below(sizeof(WORDS) / sizeof(WORDS[0]))]);
        break;
      }
      case 3: {                         // a big-endian length-like word
        if (b.size() < 4) break;
        const size_t at = r.below((uint32_t)b.size() - 3);
        const int32_t v = (int32_t)WORDS[r.below(sizeof(WORDS) / sizeof(WORDS[0]))];
        for (int s = 0; s < 4; ++s) b[at + s] = (uint8_t)((uint32_t)v >> (24 - 8 * s));
        break;
      }
      case 4: b.push_back((uint8_t)r.below(256)); break;
      default: b[r.below((uint32_t)b.size())] = (uint8_t)r.below(256);
    }
  }
}

// The loader's structural phases over one image in a heap block of exactly
// its length: (code, index).
struct Verdict { int32_t code; int64_t index; };

bool fail(const char* what, const uint8_t* p, size_t n) {
  printf("FAIL %s: ", what);
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
  printf("\n");
  return false;
}

bool run_image(const Bytes& src, Verdict* v) {
  const size_t n = src.size();
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(p, src.data(), n);
  zk::SnapHead h;
  bool ok = true;
  *v = Verdict{zk::SNAP_OK, -1};
  const int32_t rc = zk::snap_check_header(p, (int64_t)n, &h);
  if (rc != zk::SNAP_OK) {
    *v = Verdict{rc, rc == zk::SNAP_BAD_TABLE ? 0 : -1};
  } else {
    const uint8_t* tab = p + zk::SNAP_HEAD;
    const uint8_t* body = tab + 8 * (h.n + 1);
    if ((int64_t)n < zk::SNAP_HEAD + 8 * (h.n + 1) + h.body)
      ok = fail("header accepted past the image", p, n);
    for (int64_t i = 0; ok && i < h.n; ++i)
      if (!zk::snap_check_table(tab, h.n, h.body, i)) {
        *v = Verdict{zk::SNAP_BAD_TABLE, i};
        break;
      }
    for (int64_t i = 0; ok && v->code == zk::SNAP_OK && i < h.n; ++i) {
      const int64_t a = zk::ld_le64(tab + 8 * i);
      const int64_t b = zk::ld_le64(tab + 8 * (i + 1));
      // a block of the record's own: a read past the span is a report
      uint8_t* r = (uint8_t*)malloc((size_t)(b - a));
      memcpy(r, body + a, (size_t)(b - a));
      zk::SnapRec f;
      if (!zk::snap_check_record(r, b - a, &f)) {
        *v = Verdict{zk::SNAP_BAD_RECORD, i};
      } else if (f.path != 4 || f.stat != f.path + f.pl ||
                 f.data != f.stat + zk::SNAP_STAT + 4 ||
                 f.acl != f.data + f.dl || f.acl_len < 4 ||
                 f.acl + f.acl_len > b - a ||
                 zk::snap_pad8(f.acl + f.acl_len) != b - a) {
        ok = fail("record fields outside the span", r, (size_t)(b - a));
      }
      free(r);
      if (v->code != zk::SNAP_OK) break;
    }
  }
  free(p);
  return ok;
}

int fuzz(long count, uint64_t seed) {
  Rng r{seed};
  long sound = 0, refused[4] = {0, 0, 0, 0};
  for (long i = 0; i < count; ++i) {
    Bytes b = gen_image(r);
    if (!r.chance(15)) mutate(b, r);
    Verdict v;
    if (!run_image(b, &v)) return 1;
    if (v.code == zk::SNAP_OK) ++sound;
    else ++refused[v.code];
  }
  printf("fuzz: %ld images, %ld sound, refused header %ld table %ld record "
         "%ld\n", count, sound, refused[1], refused[2], refused[3]);
  return sound > 0 && refused[1] > 0 && refused[2] > 0 && refused[3] > 0 ? 0
                                                                           : 1;
}

int corpus(const char* path) {
  FILE* f = fopen(path, "rb");
  if (f == nullptr) { perror(path); return 2; }
  uint8_t lw[8];
  while (fread(lw, 1, 8, f) == 8) {
    uint64_t n = 0;
    for (int s = 0; s < 8; ++s) n |= (uint64_t)lw[s] << (8 * s);
    if (n > (1ull << 30)) { fclose(f); return 2; }
    Bytes b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != n) { fclose(f); return 2; }
    Verdict v;
    if (!run_image(b, &v)) { fclose(f); return 1; }
    printf("%d %lld\n", v.code, (long long)v.index);
  }
  fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "--fuzz") == 0)
    return fuzz(atol(argv[2]), strtoull(argv[3], nullptr, 10));
  if (argc == 3 && strcmp(argv[1], "--corpus") == 0) return corpus(argv[2]);
  fprintf(stderr, "usage: fuzz_snap --fuzz N SEED | --corpus FILE\n");
  return 2;
}
