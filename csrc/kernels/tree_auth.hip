// AUTH with `digest` identities around a session batch of any op mix
// (GpuServer.serve_sessions_mixed with perms.auth; the rule: zk_auth.h).  An
// AUTH frame (opcode 100) is no request parse_request knows: the split sends
// it to the serve, which answers it 20 bytes, BAD_ARGUMENTS, with its xid.
// Three passes around the engines, which stay as they are:
//   auth_frames_k         after the segment assign and before the ACL check:
//                         a lane per frame of the whole batch.  A frame whose
//                         opcode word is not 100 or whose segment is refused
//                         (an unsound table, a session not alive, a frame of
//                         no segment) gets res[i] = 0 and touches nothing.
//                         Otherwise auth_frame; a malformed frame, a scheme
//                         other than `digest` and credentials past AUTH_MAX
//                         bytes get res[i] = 2.  A valid frame is hashed; an
//                         identity the row holds from an earlier batch gets
//                         res[i] = 1 and writes nothing, any other claims a
//                         slot with one returning atomicAdd on cnt[row]:
//                         below AUTH_K the record is written (the id bytes,
//                         then the length) and res[i] = 1, at AUTH_K or above
//                         res[i] = 2, counted `full`.  A row found full is
//                         not added to, so cnt stays within AUTH_K plus the
//                         frames of one batch.  Two equal AUTH frames of one
//                         connection in one batch may take two slots: neither
//                         lane waits for the other's record.  (A slot goes
//                         from all zero — AuthTable.clear zeroes the records
//                         with the count — to its record once, so a lane that
//                         reads a record another lane of the batch is writing
//                         matches it only if the 28 digest bytes it sees are
//                         its own: the same identity.)
//   aclperm_check_auth_k  aclperm_check_k with aclperm_permits_auth and the
//                         identities of the frame's row; in the same launch
//                         order after auth_frames_k, so an identity holds for
//                         every frame of its connection in the batch that
//                         carries its AUTH frame.
//   auth_fix_k            where aclperm_fix_k runs, between the serve and its
//                         reply encode: a frame with res[i] != 0, of the
//                         serve's class, whose reply the serve left
//                         BAD_ARGUMENTS is answered OK (1) or AUTH_FAILED (2).
//                         The reply is the same 20 bytes with the request's
//                         xid, so the presized encode stands; a reply refused
//                         for another reason (a deferred frame) stays refused,
//                         and the frame finds its identity stored when it
//                         comes back: the pass is idempotent.
// Every read of the frame is inside rx and the frame, of the tables inside
// ncap / S, of a row inside its AUTH_K records.  No lane waits for another;
// the grids come from ncap; nothing is read back.
#include "zk_acl.h"
#include "zk_sess.h"
#include "zk_mix.h"
#include "zk_auth.h"
#include "zk_aclperm_dev.h"

namespace zk {

// stats[]: what GpuServer.auth_stats reports (AUS_ANS_*: the replies the
// fix-up wrote; a deferred frame is counted by the first four in every batch
// that carries it)
enum : int { AUS_OK = 0, AUS_FAILED = 1, AUS_FULL = 2, AUS_KNOWN = 3,
             AUS_ANS_OK = 4, AUS_ANS_FAILED = 5, AUS_N = 8 };

// The identities of row seg as a reader takes them: the count clamped to
// 0..AUTH_K (0 for a row the table does not have).
ZK_DEV int32_t auth_row_count(const ZkAuthTable& au, int64_t seg) {
  if (!sess_in(seg, au.S)) return 0;
  const int32_t c = au.cnt[seg];
  return c < 0 ? 0 : (c < AUTH_K ? c : AUTH_K);
}

__global__ __launch_bounds__(AP_T) void auth_frames_k(
    const uint8_t* __restrict__ rx, int64_t rx_len,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int32_t* __restrict__ f_seg, const int32_t* __restrict__ seg_state,
    const int64_t* __restrict__ bad, int64_t S, ZkAuthTable au,
    int32_t* __restrict__ res) {
  const int64_t i = (int64_t)blockIdx.x * AP_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  bool ok = false, failed = false, full = false, known = false;
  if (i < nf) {
    const int64_t seg = f_seg[i];
    const int64_t base = foff[i], L = flen[i];
    if (base >= 0 && L >= 8 && base <= rx_len && L <= rx_len - base &&
        ld_be32(rx + base + 4) == OP_AUTH &&
        sess_refusal(bad, seg_state, S, seg) == ERR_OK &&
        sess_in(seg, au.S)) {
      const AuthFrame f = auth_frame(rx, base, L);
      if (f.status != AF_OK) {
        failed = true;
      } else {
        const uint8_t* cred = rx + f.off;
        uint8_t b64[AUTH_B64];
        auth_digest(cred, f.n, b64);
        const int32_t ul = auth_user_len(cred, f.n);
        uint8_t* row = au.recs + seg * AUTH_ROW;
        const int32_t have = auth_row_count(au, seg);
        for (int32_t r = 0; r < have && !known; ++r)
          known = auth_identity_is(cred, ul, b64, row + r * AUTH_REC);
        if (known) {
          ok = true;
        } else if (have >= AUTH_K) {
          failed = full = true;
        } else {
          const int32_t slot = atomicAdd(&au.cnt[seg], 1);
          if (slot >= 0 && slot < AUTH_K) {
            uint8_t* rec = row + slot * AUTH_REC;
            auth_identity_put(cred, ul, b64, rec + 4);
            const int32_t il = ul + 1 + AUTH_B64;
            __builtin_memcpy(rec, &il, 4);
            ok = true;
          } else {
            failed = full = true;
          }
        }
      }
    }
    res[i] = ok ? 1 : (failed ? 2 : 0);
  }
  aclperm_count(&au.stats[AUS_OK], ok);
  aclperm_count(&au.stats[AUS_FAILED], failed);
  aclperm_count(&au.stats[AUS_FULL], full);
  aclperm_count(&au.stats[AUS_KNOWN], known);
}

__global__ __launch_bounds__(AP_T) void aclperm_check_auth_k(
    ZkTree t, ZkAclTable a, uint8_t* __restrict__ rx, int64_t rx_len,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int32_t* __restrict__ f_seg, const int32_t* __restrict__ seg_state,
    const int64_t* __restrict__ bad, int64_t S,
    const int32_t* __restrict__ addrs, ZkAuthTable au,
    int32_t* __restrict__ deny, int64_t* __restrict__ stats) {
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
            const int32_t nids = auth_row_count(au, seg);
            denied = !aclperm_permits_auth(
                a.arena + acl_off(word), acl_len(word), need.perm,
                (uint32_t)addrs[seg], au.recs + (nids > 0 ? seg * AUTH_ROW : 0),
                nids);
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

__global__ __launch_bounds__(AP_T) void auth_fix_k(
    const int32_t* __restrict__ res, const int32_t* __restrict__ cls,
    const int32_t* __restrict__ sub, const int64_t* __restrict__ n_dev,
    int64_t ncap, int32_t* __restrict__ r_err, int64_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * AP_T + threadIdx.x;
  const int64_t nd = *n_dev;
  const int64_t nf = nd < 0 ? 0 : (nd < ncap ? nd : ncap);
  bool fix = false, good = false;
  if (i < nf && res[i] != 0) {
    const int64_t j = sub[i];
    fix = cls[i] == MIX_A && sess_in(j, ncap) &&
          r_err[j] == ERR_BAD_ARGUMENTS;
    good = fix && res[i] == 1;
    if (fix) r_err[j] = good ? ERR_OK : ERR_AUTH_FAILED;
  }
  aclperm_count(&stats[AUS_ANS_OK], good);
  aclperm_count(&stats[AUS_ANS_FAILED], fix && !good);
}

static bool auth_table_ok(const ZkAuthTable* au) {
  return au != nullptr && au->recs != nullptr && au->cnt != nullptr &&
         au->stats != nullptr && au->S >= 1;
}

}  // namespace zk

extern "C" {

int64_t zk_auth_row_bytes(void) { return zk::AUTH_ROW; }

// The AUTH frames of a session batch (off / len, *n_dev of them, at most
// ncap; zk_sess_assign's table g over the whole batch) -> res[ncap] (written
// for the batch's frames: 0 no AUTH frame or a refused segment, 1 the identity
// is stored, 2 AUTH_FAILED), the identities stored in au's rows (the segment
// index is the row), au->stats[0..3] += (ok, failed, full, known).  One
// launch, no host read.
int zk_auth_frames(const uint8_t* rx, int64_t rx_len, const int64_t* foff,
                   const int32_t* flen, const int64_t* n_dev, int64_t ncap,
                   const ZkSegs* g, const ZkAuthTable* au, int32_t* res,
                   hipStream_t st) {
  if (ncap < 0 || rx_len < 0 || ncap >= 0x7fffffff)
    return (int)hipErrorInvalidValue;
  if (g == nullptr || g->f_seg == nullptr || g->seg_state == nullptr ||
      g->bad == nullptr || g->S < 1 || !zk::auth_table_ok(au) ||
      au->S < g->S)
    return -1;
  if (ncap == 0) return 0;
  zk::auth_frames_k<<<(unsigned)((ncap + zk::AP_T - 1) / zk::AP_T), zk::AP_T,
                      0, st>>>(rx, rx_len, foff, flen, n_dev, ncap, g->f_seg,
                               g->seg_state, g->bad, g->S, *au, res);
  ZK_LAUNCH_CHECK();
  return 0;
}

// zk_aclperm_check for peers that hold identities: a `digest` entry grants
// when its id is one of row f_seg[i]'s.  One launch, no host read.
int zk_aclperm_check_auth(const ZkTree* t, const ZkAclTable* a, uint8_t* rx,
                          int64_t rx_len, const int64_t* foff,
                          const int32_t* flen, const int64_t* n_dev,
                          int64_t ncap, const ZkSegs* g, const int32_t* addrs,
                          const ZkAuthTable* au, int32_t* deny, int64_t* stats,
                          hipStream_t st) {
  if (ncap < 0 || rx_len < 0 || ncap >= 0x7fffffff)
    return (int)hipErrorInvalidValue;
  if (g == nullptr || g->f_seg == nullptr || g->seg_state == nullptr ||
      g->bad == nullptr || g->S < 1 || addrs == nullptr ||
      !zk::auth_table_ok(au) || au->S < g->S)
    return -1;
  if (a->cap <= 0 || a->arena_cap <= 0) return -1;
  if (ncap == 0) return 0;
  zk::aclperm_check_auth_k<<<(unsigned)((ncap + zk::AP_T - 1) / zk::AP_T),
                             zk::AP_T, 0, st>>>(
      *t, *a, rx, rx_len, foff, flen, n_dev, ncap, g->f_seg, g->seg_state,
      g->bad, g->S, addrs, *au, deny, stats);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Between the serve of the batch's serve class and its reply encode: frame i
// of the whole batch (*n_dev of them) with res[i] != 0 and of the serve's
// class (cls[i] == 0, its reply at sub[i]), answered OK (res 1) or
// AUTH_FAILED (res 2) where the serve left BAD_ARGUMENTS in r_err[ncap];
// stats[4], stats[5] += those.  One launch, no host read.
int zk_auth_fix(const int32_t* res, const int32_t* cls, const int32_t* sub,
                const int64_t* n_dev, int64_t ncap, int32_t* r_err,
                int64_t* stats, hipStream_t st) {
  if (ncap < 0 || ncap >= 0x7fffffff) return (int)hipErrorInvalidValue;
  if (ncap == 0) return 0;
  zk::auth_fix_k<<<(unsigned)((ncap + zk::AP_T - 1) / zk::AP_T), zk::AP_T, 0,
                   st>>>(res, cls, sub, n_dev, ncap, r_err, stats);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
