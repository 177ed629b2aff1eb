// ACL enforcement around a session batch of any op mix
// (GpuServer.serve_sessions_mixed with perms; the rule: zk_aclperm.h).  The
// ACL store (tree_acl.hip) keeps every CREATE's vector; here it is read to
// decide.  Two passes around the engines, which stay as they are:
//   aclperm_check_k  after K1 and the segment assign, before the split: a
//                    lane per frame of the whole batch.  A frame the engines
//                    would refuse or not find anyway gets no verdict and is
//                    left alone: its segment is refused (a frame of no
//                    segment, an unsound table, a session not alive),
//                    parse_request rejects its body, or its target does not
//                    exist.  Otherwise: aclperm_need, one tree_lookup of the
//                    target (two for a DELETE: the node, then its parent),
//                    node_acl[target].  The open ACL's word (arena offset 0)
//                    grants without a read of the arena: the path almost
//                    every node takes.  A lost binding (ACL_LOST, or a word
//                    acl_word_ok rejects) denies: closed, and counted apart.
//                    Anything else walks its bytes (aclperm_permits) for the
//                    peer address of the frame's segment.
//                    A denied frame gets deny[i] = 1 and its opcode word in
//                    rx overwritten with OP_UNKNOWN: the split sends such a
//                    frame to the serve, the SEQUENTIAL numbering and the
//                    ordering see no request in it, and the serve answers it
//                    20 bytes, BAD_ARGUMENTS, with its xid, having looked up,
//                    claimed, armed and fired nothing.
//   aclperm_fix_k    between the serve and its reply encode (where
//                    cl_frames_k runs): a lane per frame of the whole batch;
//                    a denied frame whose reply the serve left BAD_ARGUMENTS
//                    is answered NO_AUTH.  The reply is the same 20 bytes, so
//                    the presized encode stands.  A reply refused for another
//                    reason (a deferred frame, a rank the passes cannot
//                    reach) stays refused; a frame that came with an opcode
//                    of no request was never marked.
// Every read of the frame is inside rx and the frame, of the tables inside
// ncap / S / the node capacity, of the arena inside arena_cap.  No lane waits
// for another; the grids come from ncap; nothing is read back.  The counters
// go up by one atomic a wave each, as sess_assign_k's.
#include "zk_acl.h"
#include "zk_sess.h"
#include "zk_mix.h"
#include "zk_aclperm.h"
#include "zk_aclperm_dev.h"

namespace zk {

__global__ __launch_bounds__(AP_T) void aclperm_check_k(
    ZkTree t, ZkAclTable a, uint8_t* __restrict__ rx, int64_t rx_len,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int32_t* __restrict__ f_seg, const int32_t* __restrict__ seg_state,
    const int64_t* __restrict__ bad, int64_t S,
    const int32_t* __restrict__ addrs, int32_t* __restrict__ deny,
    int64_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * AP_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  bool checked = false, denied = false, lost = false;
  if (i < nf) {
    const int64_t seg = f_seg[i];
    const int64_t base = foff[i], L = flen[i];
    if (sess_refusal(bad, seg_state, S, seg) == ERR_OK && base >= 0 &&
        L >= 8 && base <= rx_len && L <= rx_len - base) {
      const ReqFields rq = parse_request(rx, base, L);
      const AclNeed need = aclperm_need(rq.op);
      if (rq.status == ST_OK && need.target != ACLT_NONE && rq.poff >= 0) {
        const int64_t node = aclperm_target(t, rx, rq, need.target);
        if (node >= 0 && node < a.cap && node < t.store.cap) {
          checked = true;
          const int64_t word = a.node_acl[node];
          if (!acl_word_ok(a, word)) {
            denied = lost = true;
          } else if (acl_off(word) != 0) {         // (0: the open ACL)
            denied = !aclperm_permits(a.arena + acl_off(word), acl_len(word),
                                      need.perm, (uint32_t)addrs[seg]);
          }
          if (denied) st_be32(rx + base + 4, OP_UNKNOWN);
        }
      }
    }
    deny[i] = denied ? 1 : 0;
  }
  aclperm_count(&stats[APS_CHECKED], checked);
  aclperm_count(&stats[APS_DENIED], denied);
  aclperm_count(&stats[APS_DENIED_LOST], lost);
}

__global__ __launch_bounds__(AP_T) void aclperm_fix_k(
    const int32_t* __restrict__ deny, const int32_t* __restrict__ cls,
    const int32_t* __restrict__ sub, const int64_t* __restrict__ n_dev,
    int64_t ncap, int32_t* __restrict__ r_err, int64_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * AP_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  bool fix = false;
  if (i < nf && deny[i] != 0) {
    const int64_t j = sub[i];
    fix = cls[i] == MIX_A && sess_in(j, ncap) &&
          r_err[j] == ERR_BAD_ARGUMENTS;
    if (fix) r_err[j] = ERR_NO_AUTH;
  }
  aclperm_count(&stats[APS_ANSWERED], fix);
}

}  // namespace zk

extern "C" {

// The verdicts of a session batch's frames (off / len, *n_dev of them, at most
// ncap; zk_sess_assign's table g over the whole batch) against the ACLs the
// tree holds as the batch finds it, for the peers addrs[S] (host-order IPv4,
// 0: none) -> deny[ncap] (written for the batch's frames), the denied frames'
// opcode words in rx overwritten, stats[8] += (checked, denied, denied for a
// lost binding).  One launch, no host read.
int zk_aclperm_check(const ZkTree* t, const ZkAclTable* a, uint8_t* rx,
                     int64_t rx_len, const int64_t* foff, const int32_t* flen,
                     const int64_t* n_dev, int64_t ncap, const ZkSegs* g,
                     const int32_t* addrs, int32_t* deny, int64_t* stats,
                     hipStream_t st) {
  if (ncap < 0 || rx_len < 0 || ncap >= 0x7fffffff)
    return (int)hipErrorInvalidValue;
  if (g == nullptr || g->f_seg == nullptr || g->seg_state == nullptr ||
      g->bad == nullptr || g->S < 1 || addrs == nullptr)
    return -1;
  if (a->cap <= 0 || a->arena_cap <= 0) return -1;
  if (ncap == 0) return 0;
  zk::aclperm_check_k<<<(unsigned)((ncap + zk::AP_T - 1) / zk::AP_T), zk::AP_T,
                        0, st>>>(*t, *a, rx, rx_len, foff, flen, n_dev, ncap,
                                 g->f_seg, g->seg_state, g->bad, g->S, addrs,
                                 deny, stats);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Between the serve of the batch's serve class and its reply encode: frame i
// of the whole batch (*n_dev of them), denied (deny[i]) and of the serve's
// class (cls[i] == 0, its reply at sub[i]), answered NO_AUTH where the serve
// left BAD_ARGUMENTS in r_err[ncap]; stats[3] += those.  One launch, no host
// read.
int zk_aclperm_fix(const int32_t* deny, const int32_t* cls, const int32_t* sub,
                   const int64_t* n_dev, int64_t ncap, int32_t* r_err,
                   int64_t* stats, hipStream_t st) {
  if (ncap < 0 || ncap >= 0x7fffffff) return (int)hipErrorInvalidValue;
  if (ncap == 0) return 0;
  zk::aclperm_fix_k<<<(unsigned)((ncap + zk::AP_T - 1) / zk::AP_T), zk::AP_T,
                      0, st>>>(deny, cls, sub, n_dev, ncap, r_err, stats);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
