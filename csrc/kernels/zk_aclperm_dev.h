// What the ACL check's kernels share (tree_aclperm.hip, tree_auth.hip): the
// block size, the counters, the one-atomic-a-wave count and the lookup of the
// node whose ACL decides.  Device code; the rule itself is zk_aclperm.h.
#pragma once
#include "zk_acl.h"
#include "zk_aclperm.h"

namespace zk {

constexpr int AP_T = 256;

// stats[]: what GpuServer.acl_enforce_stats reports
// (APS_ANSWERED: the replies the fix-up turned into NO_AUTH — a denied frame
// that the ordered serve defers is checked again in the batch that serves it)
enum : int { APS_CHECKED = 0, APS_DENIED = 1, APS_DENIED_LOST = 2,
             APS_ANSWERED = 3, APS_N = 8 };

ZK_DEV void aclperm_count(int64_t* __restrict__ ctr, bool mine) {
  const uint64_t m = __ballot(mine);
  if (m != 0 && lane_id() == __ffsll((unsigned long long)m) - 1)
    atomicAdd((unsigned long long*)ctr, (unsigned long long)__popcll(m));
}

// The node whose ACL decides request rq, or -1: no verdict.
ZK_DEV int64_t aclperm_target(const ZkTree& t, const uint8_t* __restrict__ rx,
                              const ReqFields& rq, int32_t target) {
  const uint8_t* p = rx + rq.poff;
  if (target == ACLT_NODE) return tree_lookup(t, p, rq.pl).node;
  if (target == ACLT_PARENT_OF_NODE && tree_lookup(t, p, rq.pl).node < 0)
    return -1;
  const int32_t cut = aclperm_parent_cut(p, rq.pl);
  return cut > 0 ? tree_lookup(t, p, cut).node : -1;
}

}  // namespace zk
