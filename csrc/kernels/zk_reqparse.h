// Server-mode request parse (K12), shared by decode_requests_k (SoA output)
// and the GPU server's fused serve (csrc/kernels/tree.hip), which parses
// each frame in registers instead of reading the SoA back.
// Reference: lib/zk-buffer.js:58-253 (request layouts).
//
// skip_strings / skip_acl / parse_request live in zk_wire.h, which has no
// HIP include: the host compiler builds the same text for the sanitizer
// harness (tools/fuzz_reqparse.cpp).
#pragma once
#include "zk_common.h"
#include "zk_wire.h"
