// The index arithmetic of the consumers' frame staging (zk_frame_rows.h
// fr_span_load, fr_span_store) in plain C++: no HIP include, so the host compiler builds
// the very text the kernels run (tools/stage_span_host.cpp puts it under
// ASan + UBSan on a machine without a GPU).
//
// A wave's frames are one contiguous span [s, e) of the stream buf[0, n).
// Its image is the run of 16-byte chunks, aligned as ADDRESSES, that covers
// the span: chunk c holds the stream bytes [off0 + 16 c, off0 + 16 c + 16),
// stream byte s lies at image byte `head`.  The first chunk may start before
// the buffer (an unaligned buf and s < 16) and the last may end past n (the
// stream's end): such a chunk is loaded byte by byte, clipped to [0, n), and
// its other bytes are zero.  No byte outside buf[0, n) is ever read.
#pragma once
#include <stdint.h>

#include "zk_wire.h"   // ZK_HD

namespace zk {

struct StageSpan {
  int64_t off0;      // stream offset of chunk 0 (negative: before the buffer)
  int32_t head;      // image offset of stream byte s (0..15)
  int32_t nchunks;   // 16-byte chunks of the image
  bool clipped;      // a chunk leaves [0, n)
};

// Is [s, e) a span of a stream of n bytes, of at most `budget` bytes?
ZK_HD bool span_fits(int64_t s, int64_t e, int64_t n, int64_t budget) {
  return s >= 0 && s <= e && e <= n && e - s <= budget;
}

// base: the ADDRESS of stream byte 0 (only its low four bits matter).
// Requires span_fits(s, e, n, ·).
ZK_HD StageSpan span_make(uint64_t base, int64_t s, int64_t e, int64_t n) {
  StageSpan sp;
  sp.head = (int32_t)((base + (uint64_t)s) & 15);
  sp.off0 = s - sp.head;
  sp.nchunks = (int32_t)((sp.head + (e - s) + 15) >> 4);
  sp.clipped = sp.off0 < 0 || sp.off0 + 16 * (int64_t)sp.nchunks > n;
  return sp;
}

// Do the span's chunks fit an image of img_bytes (a multiple of 16)?  The
// head's misalignment counts: a span of img_bytes - 15 always fits.
ZK_HD bool span_image_fits(const StageSpan& sp, int64_t img_bytes) {
  return 16 * (int64_t)sp.nchunks <= img_bytes;
}

ZK_HD int64_t span_chunk_off(const StageSpan& sp, int32_t c) {
  return sp.off0 + 16 * (int64_t)c;
}

// Chunk c (< nchunks) as four dwords in memory order.
ZK_HD void span_load_chunk(const uint8_t* buf, int64_t n, const StageSpan& sp,
                           int32_t c, uint32_t (&w)[4]) {
  const int64_t g = span_chunk_off(sp, c);
  if (g >= 0 && g + 16 <= n) {
    __builtin_memcpy(w, buf + g, 16);
    return;
  }
  w[0] = w[1] = w[2] = w[3] = 0;
  for (int k = 0; k < 16; ++k)
    if (g + k >= 0 && g + k < n)
      w[k >> 2] |= (uint32_t)buf[g + k] << (8 * (k & 3));
}

}  // namespace zk
