// The session table's slot rule (ZkSessionTable, zk_abi.h), shared by the
// handshake (session.hip) and the session batches' liveness check
// (tree_sess.hip).
#pragma once
#include "zk_common.h"

namespace zk {

enum : int32_t { SS_FREE = 0, SS_ALIVE = 1, SS_CLOSED = 2 };

// The table slot of session id s (-1: not one this table can hold).
ZK_DEV int64_t sess_slot(const ZkSessionTable& tab, int64_t s,
                         int64_t server_id) {
  const int64_t srv = (s >> 56) & 0x7f;
  const int64_t idx = (s & 0x00ffffffffffffffll) - 1;
  if (idx < 0) return -1;
  if (tab.span == 0) return srv == server_id && idx < tab.cap ? idx : -1;
  if (srv < 1 || idx >= tab.span || srv * tab.span > tab.cap) return -1;
  return (srv - 1) * tab.span + idx;
}

}  // namespace zk
