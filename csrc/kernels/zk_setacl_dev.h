// What the SET_ACL pass (tree_setacl.hip) and the ACL engine's launcher
// (tree_acl.hip zk_tree_acl_setacl_sessions) share: the pass's workspace, its
// counters and the host functions through which the launcher starts the
// pass's kernels.  Device code; the rule itself is zk_setacl.h.
#pragma once
#include "zk_acl.h"
#include "zk_sess.h"
#include "zk_setacl.h"

namespace zk {

static_assert(SETACL_VEC_MAX == ACL_LEN_MAX, "one limit for a stored vector");

// stats[]: what GpuServer.setacl_stats reports
enum : int { SAS_APPLIED = 0, SAS_BAD_VERSION = 1, SAS_DENIED = 2,
             SAS_INVALID = 3, SAS_UNREACHED = 4, SAS_STORE_FULL = 5,
             SAS_N = 8 };

// A frame of the class's table to the pass: none of its frames (another
// opcode, a refused segment: the row acl_size_sess_k wrote stands), answered,
// or past every check but the version and waiting for its node.
enum : int32_t { SS_NONE = 0, SS_FINAL = 1, SS_PEND = 2 };

// The idle value of a node's claim word (the owner fills the table with it
// once; every round's winner puts it back).
constexpr int32_t SETACL_IDLE = 0x7fffffff;

struct SetAclWs {
  int64_t* ctr;                 // [8] 0: the zxids the pass takes
  int32_t* state;               // [ncap] SS_*
  int32_t* err;                 // [ncap] the answer of an SS_FINAL frame
  int32_t* xid;                 // [ncap]
  int32_t* ver;                 // [ncap] the frame's version
  int32_t* vlen;                // [ncap] bytes of its vector
  int32_t* islot;               // [ncap] the intern index slot / AS_*
  int32_t* aver;                // [ncap] the aversion the frame produced
  int64_t* node;                // [ncap]
  int64_t* nslot;               // [ncap] the node's slot offset
  int64_t* voff;                // [ncap] the vector's offset in rx
  int64_t* word;                // [ncap] its arena word
  int64_t* zflag;               // [ncap] 1: the frame takes a zxid
  int64_t* zoff;                // [ncap] the exclusive scan of zflag
  int64_t* scan;                // zk_scan_workspace(ncap)
};

// The ACL engine's rows (tree_acl.hip AclWs) the pass overwrites for its
// frames, and the word acl_total_k leaves (!= 0: nothing is written).
struct SetAclRows {
  int32_t* xid;
  int32_t* err;
  int64_t* word;
  int64_t* nslot;
  int64_t* sizes;
  const int64_t* over;
};

int64_t setacl_layout(int64_t ncap, uint8_t* ws, SetAclWs* w);

// judge + intern, the P rounds: before the class's GET_ACL frames are sized
int setacl_pass(const ZkTree& t, const ZkAclTable& a, const uint8_t* rx,
                int64_t rx_len, const int64_t* foff, const int32_t* flen,
                const int64_t* n_dev, int64_t ncap, const SegTable& M,
                const int32_t* addrs, const ZkAuthTable* au, int32_t passes,
                int32_t* claim, const SetAclWs& w, int64_t* stats,
                hipStream_t st);
// after acl_size_sess_k: the pass's frames into the engine's rows, the zxids
int setacl_rows(const int64_t* n_dev, int64_t ncap, const SetAclWs& w,
                const SetAclRows& r, int64_t* stats, hipStream_t st);
// after the class's scan and acl_total_k: every reply of the class, then the
// tree's zxid counter
int setacl_write(const ZkTree& t, const ZkAclTable& a, const int64_t* n_dev,
                 int64_t ncap, const SetAclWs& w, const SetAclRows& r,
                 const int64_t* rec_off, uint8_t* out, hipStream_t st);

}  // namespace zk
