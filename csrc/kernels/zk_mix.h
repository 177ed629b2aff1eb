// The engine class of a request frame in a mixed batch (tree_mix.hip), in
// plain C++ like zk_wire.h: the host compiler builds the very text the split
// kernel runs (tools/mix_class_host.cpp puts it under ASan + UBSan on a
// machine without a GPU).
#pragma once
#include "zk_wire.h"

namespace zk {

// The classes in engine order (GpuServer.serve_mixed runs them so): A the
// fused serve, C the GET_ACL engine, L the list engine.
enum : int32_t { MIX_A = 0, MIX_C = 1, MIX_L = 2, MIX_CLASSES = 3 };

// Frame body [base, base + L) of buf -> its class, from the opcode word
// (bytes 4..8 of the body) alone.  A truncated list or GET_ACL frame stays
// with its engine (which answers BAD_ARGUMENTS); a frame without an opcode
// word, any other opcode, and GET_ACL on a tree without an ACL table go to
// the serve (BAD_ARGUMENTS / UNIMPLEMENTED there).
ZK_HD int32_t mix_class(const uint8_t* __restrict__ buf, int64_t base,
                        int64_t L, bool has_acl) {
  if (L < 8) return MIX_A;
  const int32_t op = ld_be32(buf + base + 4);
  if (op == OP_GET_CHILDREN || op == OP_GET_CHILDREN2) return MIX_L;
  if (op == OP_GET_ACL && has_acl) return MIX_C;
  return MIX_A;
}

// The second rule, for a caller that serves SET_ACL
// (GpuServer.serve_sessions_mixed with setacl): mix_class, but opcode 7 is of
// the ACL engine's class on a tree with an ACL table, whatever stands behind
// the opcode word (the pass there answers a truncated frame).  Without an ACL
// table it stays with the serve.
ZK_HD int32_t mix_class_setacl(const uint8_t* __restrict__ buf, int64_t base,
                               int64_t L, bool has_acl) {
  if (L >= 8 && has_acl && ld_be32(buf + base + 4) == OP_SET_ACL) return MIX_C;
  return mix_class(buf, base, L, has_acl);
}

}  // namespace zk
