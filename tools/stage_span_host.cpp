// The consumers' frame staging on the host — csrc/kernels/zk_stage_span.h
// span_fits / span_make / span_load_chunk, the text zk_frame_rows.h
// fr_span_load and fr_span_store run — a stand-alone program for ASan + UBSan
// (tests/test_stage_span_host.py):
//   stage_span_host <budget> <span> [<span> ...]
// For every span length, every head alignment 0..15 of the stream's address,
// every span start in {0, 1, 5, 15, 16, 37} and every tail 0..15 (bytes of
// stream after the span), the span is copied chunk by chunk from a heap block
// of EXACTLY the stream's length into an image, as a wave's lanes do, and the
// image is compared with a byte-wise copy.  A read one byte outside the
// stream is a sanitizer report.  The block's own address is 16-byte aligned;
// the alignment under test is the `base` handed to span_make, which is all
// the arithmetic sees of the address.  <budget> is the image's bytes: a case
// is staged when the span with its head fits it (span_fits and
// span_image_fits, as the kernels decide).  Prints "<span> <cases staged>" a
// span (of 6 * 16 * 16); exits 1 on a mismatch.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc/kernels \
//       tools/stage_span_host.cpp -o stage_span_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_stage_span.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <budget> <span> [<span> ...]\n", argv[0]);
    return 2;
  }
  const int64_t budget = std::atoll(argv[1]);
  const int64_t starts[] = {0, 1, 5, 15, 16, 37};
  for (int a = 2; a < argc; ++a) {
    const int64_t span = std::atoll(argv[a]);
    if (span < 0 || span > (1 << 24)) return 2;
    long cases = 0;
    for (int64_t s : starts)
      for (int tail = 0; tail < 16; ++tail) {
        const int64_t e = s + span, n = e + tail;
        uint8_t* buf = (uint8_t*)std::malloc(n > 0 ? (size_t)n : 1);
        for (int64_t k = 0; k < n; ++k)
          buf[k] = (uint8_t)(k * 131 + (k >> 8) * 7 + 1);
        for (uint64_t base = 0; base < 16; ++base) {
          if (!zk::span_fits(s, e, n, budget)) continue;
          const zk::StageSpan sp = zk::span_make(base, s, e, n);
          if (!zk::span_image_fits(sp, budget)) continue;
          // the image the kernels reserve: budget bytes of chunks
          if (sp.head < 0 || sp.head > 15 ||
              16 * (int64_t)sp.nchunks > budget ||
              sp.head + span > 16 * (int64_t)sp.nchunks) {
            std::fprintf(stderr, "span %lld: image out of range\n",
                         (long long)span);
            return 1;
          }
          std::vector<uint8_t> img((size_t)16 * sp.nchunks + 1, 0xEE);
          for (int32_t c = 0; c < sp.nchunks; ++c) {
            uint32_t w[4];
            zk::span_load_chunk(buf, n, sp, c, w);
            std::memcpy(img.data() + 16 * c, w, 16);
          }
          for (int64_t k = 0; k < span; ++k)
            if (img[(size_t)(sp.head + k)] != buf[s + k]) {
              std::fprintf(stderr, "span %lld base %d s %lld tail %d: byte "
                           "%lld differs\n", (long long)span, (int)base,
                           (long long)s, tail, (long long)k);
              return 1;
            }
          // unclipped: every chunk lies inside the stream
          if (!sp.clipped &&
              (sp.off0 < 0 || sp.off0 + 16 * (int64_t)sp.nchunks > n)) {
            std::fprintf(stderr, "span %lld: clipped not set\n",
                         (long long)span);
            return 1;
          }
          ++cases;
        }
        std::free(buf);
      }
    std::printf("%lld %ld\n", (long long)span, cases);
  }
  return 0;
}
