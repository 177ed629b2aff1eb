// The host/device ABI of libzkmi_hip.so, in ONE place: every descriptor
// struct a launcher takes and every extern "C" launcher prototype.  The
// kernel sources (through zk_common.h) and the torch operator library
// (csrc/torch/zkmi_ops.cpp) both include it, so a launcher whose definition
// drifts from its prototype does not compile (C linkage cannot overload),
// and the static_asserts below pin each struct's layout on both compilers
// (hipcc for the kernels, g++ for the op library).  The build stamps of both
// libraries hash this file (tools/build_native.py).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

extern "C" {


// K10 — request descriptors (SoA).  `arg` is watch (GET_DATA / EXISTS /
// GET_CHILDREN*), flags (CREATE) or version (DELETE / SET_DATA).  Lengths < 0
// mean "empty" and go on the wire as -1.
struct ZkReqBatch {
  const int32_t* opcode;
  const int32_t* xid;
  const int32_t* arg;
  const int64_t* path_off;
  const int32_t* path_len;
  const int64_t* data_off;
  const int32_t* data_len;
  const int32_t* acl_id;
  const uint8_t* path_arena;
  const uint8_t* data_arena;
  const int64_t* acl_off;   // pre-encoded ACL vectors (count + entries)
  const int32_t* acl_len;
  const uint8_t* acl_arena;
};

// Node store of the GPU-resident synthetic server (HBM).  Each node owns a
// 16-byte aligned slot in `slab` laid out in WIRE format, so a reply is two
// contiguous copies, not 13 field gathers from SoA arrays (a random node is
// then 2-3 cache lines instead of ~13):
//   [0,68)   Stat, big-endian (version at +32, 4-byte aligned for CAS)
//   [72,76)  data length, big-endian (-1 when empty, as Jute writes it)
//   [76,..)  data bytes (capacity slot_cap)
struct ZkNodeStore {
  uint8_t* slab;
  int64_t* slot_off;  // [cap] byte offset of the node's slot in slab
  int32_t* data_len;  // [cap] host-endian copy of the data length
  int32_t* slot_cap;  // [cap] data capacity of the slot
  int64_t cap;
};
#define ZK_SLOT_STAT 0
#define ZK_SLOT_LEN 72
#define ZK_SLOT_DATA 76

// K13 — reply descriptors for server-mode encode.
struct ZkRespBatch {
  const int32_t* opcode;
  const int32_t* xid;
  const int32_t* err;
  const int64_t* node;      // node index (stat / data source), -1 if none
  const int64_t* zxid;
  const int64_t* path_off;  // CREATE reply path / NOTIFICATION path
  const int32_t* path_len;
  const uint8_t* path_arena;
  const int32_t* aux;       // NOTIFICATION type
  const int64_t* slot;      // node's slot offset in the slab (null: look
                            // it up through node -> slot_off)
};

// K2-K8 — decoded replies (SoA, `cap` rows).
struct ZkReplyOut {
  int32_t* xid;
  int32_t* err;
  int32_t* opcode;
  int32_t* status;
  int64_t* zxid;
  int64_t* stat64;   // [6][cap]
  int32_t* stat32;   // [5][cap]
  int64_t* pay_off;  // data / created path / notification path / vector region
  int32_t* pay_len;
  int32_t* aux0;     // notification type | child / acl count
  int32_t* aux1;     // notification state
  int64_t cap;
};

// K12 — decoded requests (server mode).
struct ZkReqOut {
  int32_t* xid;
  int32_t* opcode;
  int32_t* status;
  int64_t* path_off;
  int32_t* path_len;
  int64_t* data_off;
  int32_t* data_len;
  int32_t* arg;       // watch / version / flags
  int64_t* vec_off;   // CREATE: ACL region; SET_WATCHES: first vector
  int32_t* vec_count; // CREATE: ACL entries; SET_WATCHES: total paths
  int64_t* rel_zxid;  // SET_WATCHES
  int64_t cap;
};

// tree_serve_k's reply descriptors for K13 (ncap rows; block_sums:
// ceil(ncap / 256)).  slot may be null; sizes and block_sums may be null,
// both or neither.
struct ZkServeOut {
  int32_t *opcode, *xid, *err;
  int64_t *node, *zxid, *path_off;
  int32_t* path_len;
  int64_t *slot, *sizes, *block_sums;
};

// The segment table of a session batch (tree_sess.hip; the rule: zk_sess.h):
// zk_sess_assign's f_seg / seg_state / bad and the caller's sessions / wslots.
// Every engine of a session batch takes it in place of one session and one
// watcher slot; the list, GET_ACL and catch-up engines read no sessions, the
// GET_ACL engine no wslots.
struct ZkSegs {
  const int32_t* f_seg;      // [ncap] frame -> segment (of the whole batch,
                             // or of one class: zk_sess_split_segments)
  const int64_t* sessions;   // [S]
  const int32_t* wslots;     // [S]
  const int32_t* seg_state;  // [S] 0 serve, 1 session not alive
  const int64_t* bad;        // [2] != 0: the table is unsound
  int64_t S;
};

// Deferral in the ordered session serve (tree_order.hip ord_clip_*; the rules:
// zk_order_clip.h), over the WHOLE batch of any op mix: the split's cls / sub,
// its frame count, the assign's f_seg and the three classes' segment tables ->
// the deferred frames' entries of f_seg / seg_c become -1, clipf[S] (per
// segment the first deferred whole-batch frame; ncap: none), deferred[1].
struct ZkOrdClip {
  const int32_t* cls;      // [ncap] the split's class per frame
  const int32_t* sub;      // [ncap] its index in the class's table
  const int64_t* nall;     // the whole batch's frame count
  int32_t* f_seg;          // [ncap] frame -> segment (deferred: -1)
  int32_t* seg_c[3];       // [ncap] each class's frame -> segment
  int64_t* clipf;          // [S] first deferred frame (ncap: none)
  int64_t* deferred;       // [1] frames deferred
  const int64_t* bad;      // the table's fault word (or null): != 0, the batch
  int64_t S;               // is refused as a whole and nothing is deferred
};

// The GPU-resident synthetic server's tree (zk_tree.h; kernels in tree.hip
// and tree_{order,seq,list,watch}.hip).
struct ZkTree {
  int64_t* ht;                 // [2 * (mask + 1)] interleaved {key, val}
  int64_t mask;
  int64_t* node_path_off;
  int32_t* node_path_len;
  int64_t* node_parent;        // parent node index, -1 = root, -2 = free
  uint8_t* path_arena;
  int64_t path_cap;
  int64_t slab_cap;
  int64_t* counters;           // see TC_* below
  ZkNodeStore store;
  int64_t* free_list;          // ring of deleted node indices
  int64_t free_cap;
  // [cap] cversion << 32 | numChildren, host-endian: a child's create or
  // delete updates both with one atomic
  int64_t* cn;
  int64_t* pzxid;              // [cap] host-endian pzxid
  int32_t* dirty;              // [cap] parent-on-dirty-list flag
  int64_t* dirty_list;         // [cap]
  int64_t* node_pw;            // [cap] path word: offset << 24 | length
  int32_t* node_path_cap;      // [cap] bytes of the node's path storage
  int64_t* eph;                // [cap] host-endian ephemeralOwner shadow
  // watch table (null wt_key: the tree keeps no watches), see wt_* below
  // [2 * (wt_hmask + 1)]: per entry the path hash | 1 (0 = empty) and the
  // path's second hash | 1 (0 = not yet published), side by side
  int64_t* wt_key;
  // [2 * (wt_hmask + 1) + WT_STATS]: data / child masks, then the counters
  // (WS_*: arms that found no entry)
  unsigned long long* wt_mask;
  int64_t wt_hmask;
  // [ncap] per request of the batch being served: its parent node << 32 |
  // its SEQUENTIAL number, assigned in stream order by zk_tree_seq_order
  // (-1: none; the serve then takes the parent's cversion atomically).
  // Null: no request has one.
  const int64_t* seqno;
};

// Server-side session table (session.hip, K9 server mode).
struct ZkSessionTable {
  int64_t* sid;       // [cap]
  uint8_t* passwd;    // [cap * 16]
  int32_t* timeout;   // [cap]
  int32_t* state;     // [cap] SS_*
  int64_t* next;      // [1] allocation counter
  int64_t cap;
  // 0: one server's table (slot = the id's index).  > 0: an ensemble's
  // replicated table, `span` slots per member: the session with id
  // (member << 56 | index + 1) lives at slot (member - 1) * span + index
  int64_t span;
};

// ACL store beside the tree (tree_acl.hip).  ZkTree itself keeps no ACL: a
// CREATE's vector is interned here by a pass after the serve, and GET_ACL
// batches read node_acl -> arena.
struct ZkAclTable {
  // [cap] per node: arena offset << 24 | byte length of its ACL vector in
  // wire format (be32 count + entries); -1: lost (the store was full)
  int64_t* node_acl;
  int64_t cap;
  uint8_t* arena;     // the interned vectors, each once; the open ACL at 0
  int64_t arena_cap;
  // intern index (open addressing, create time only): content hash | 1
  // (0 = empty) -> the vector's arena word (0 = being published, -1 = lost)
  int64_t* key;       // [hmask + 1]
  int64_t* val;       // [hmask + 1]
  int64_t hmask;
  // [8] arena top, entries, nodes bound lost, the arena top after the last
  // record pass, the entry limit
  int64_t* ctr;
};

// The identities the connections of a session batch hold after AUTH
// (tree_auth.hip; the rule and the record layout: zk_auth.h).  ZooKeeper keeps
// authentication per connection, so the row is the segment index.
struct ZkAuthTable {
  // [S * zk_auth_row_bytes()] per row 4 records of 160 bytes: the id's length
  // (native int32), then up to 148 id bytes
  uint8_t* recs;
  int32_t* cnt;       // [S] records claimed in the row (readers clamp to 4)
  int64_t* stats;     // [8] ok, failed, full, known, answered OK / AUTH_FAILED
  int64_t S;
};

// K1's per-tile frame-start lists, as a consumer of a rows-deferred scan
// (zk_frame_scan flags bit 24) reads them: zk_frame_rows.h turns a
// workgroup's 256 frames into (body offset, length) rows from these, and
// clears the scan's flag words for the next scan of the workspace.
// zk_frame_tiles fills it from the workspace a scan ran on.
struct ZkFrameTiles {
  const uint8_t* buf;        // the stream
  const int64_t* n_dev;      // its device length (null: n_cap)
  int64_t n_cap;
  const uint16_t* list;      // [tiles][1024] frame starts of the tile's chain
  const uint16_t* pre;       // [tiles][1024] starts walked before joining it
  const int64_t* rec_meta;   // [tiles] cnt | np | js | term | bad | stale
  const int64_t* rec_entry;  // [tiles]
  const int64_t* rec_exit;   // [tiles]
  const int64_t* base;       // [tiles] row base within the tile's count block
  const int64_t* bsum;       // [tiles / 64 + 1] row base of the count block
  const int64_t* lastk;      // [1] the last live tile (-1: no frame)
  // [4 * tiles + 1] per block of 256 frames: the count block (64 tiles)
  // holding the tile in which frame 256 j starts (fs_link's last workgroup)
  const int32_t* fblk;
  uint64_t* lbw;             // flag words: two a tile, then the LW_* tail
  int64_t tiles;             // of the workspace's layout (n_cap's)
};

// ---- launchers (stream-ordered; return 0 or a hipError_t) ----------------
int64_t zk_scan_workspace(int64_t n);
int zk_scan_set_mode(int mode);
// the one-workgroup exclusive scan with an explicit engine (1 MFMA, 0 shfl)
int zk_scan_small_i64_mode(const int64_t*, int64_t*, int64_t, int64_t*, int,
                           hipStream_t);
int zk_scan_excl_i64(const int64_t*, int64_t*, int64_t, int64_t*, int64_t*,
                     hipStream_t);
int zk_scan_excl_i32(const int32_t*, int64_t*, int64_t, int64_t*, int64_t*,
                     hipStream_t);
int zk_encode_requests(const ZkReqBatch*, int64_t, int64_t*, int64_t*,
                       int64_t*, int64_t*, uint8_t*, int64_t, int64_t*,
                       int64_t, int32_t*, int32_t, hipStream_t);
int zk_encode_requests_presized(const ZkReqBatch*, int64_t, const int64_t*,
                                const int64_t*, int64_t*, int64_t*, int64_t*,
                                uint8_t*, int64_t, int64_t*, int64_t,
                                int32_t*, int32_t, hipStream_t);
int zk_encode_set_watches(const int64_t*, const int32_t*, const uint8_t*,
                          int64_t, int64_t, int64_t, int64_t, int64_t*,
                          int64_t*, int64_t*, int64_t*, uint8_t*, int64_t,
                          int32_t*, hipStream_t);
int zk_encode_connect_requests(const int32_t*, const int64_t*, const int32_t*,
                               const int64_t*, const int64_t*, const int32_t*,
                               const uint8_t*, int64_t, int64_t*, int64_t*,
                               int64_t*, int64_t*, uint8_t*, hipStream_t);
int zk_encode_responses(const ZkRespBatch*, const ZkNodeStore*,
                        const int64_t*, int64_t, int64_t*, int64_t*,
                        int64_t*, int64_t*, uint8_t*, int64_t, int32_t*,
                        int32_t, int32_t, hipStream_t);
int64_t zk_frame_scan_workspace(int64_t n);
int zk_frame_scan(const uint8_t*, const int64_t*, int64_t, int64_t,
                  uint8_t*, int64_t, int64_t*, int32_t*, int64_t, int64_t*,
                  int32_t, int32_t, int32_t, hipStream_t);
int zk_frame_scan_stats(const uint8_t*, int64_t, uint32_t*, hipStream_t);
int zk_frame_scan_dbg(int64_t* host, int64_t tiles);
// the tile lists of the scan of buf[0, min(*n_dev, n_cap)) on workspace ws
// (-1: workspace too small; -2: a stream of one tile at most has none)
int zk_frame_tiles(const uint8_t* buf, const int64_t* n_dev, int64_t n_cap,
                   uint8_t* ws, int64_t ws_bytes, ZkFrameTiles* out);
// zk_decode_replies / _check after a rows-deferred scan: the rows come from
// the tile lists and are also written to foff / flen [ncap]
int zk_decode_replies_tiles(const ZkFrameTiles*, int64_t*, int32_t*,
                            const int64_t*, int64_t, const int64_t*, int64_t,
                            const ZkReplyOut*, hipStream_t);
int zk_decode_replies_check_tiles(const ZkFrameTiles*, int64_t*, int32_t*,
                                  const int64_t*, int64_t, const int64_t*,
                                  int64_t, const ZkReplyOut*, const int64_t*,
                                  const int32_t*, const int32_t*,
                                  unsigned long long*, int32_t, int64_t*,
                                  const uint8_t*, const int64_t*,
                                  hipStream_t);
int zk_decode_replies(const uint8_t*, const int64_t*, const int32_t*,
                      const int64_t*, int64_t, const int64_t*, int64_t,
                      const ZkReplyOut*, hipStream_t);
int zk_decode_replies_check(const uint8_t*, const int64_t*, const int32_t*,
                            const int64_t*, int64_t, const int64_t*, int64_t,
                            const ZkReplyOut*, const int64_t*, const int32_t*,
                            const int32_t*, unsigned long long*, int32_t,
                            int64_t*, const uint8_t*, const int64_t*,
                            hipStream_t);
int zk_expand_strings(const uint8_t*, const int64_t*, const int32_t*,
                      const int64_t*, int64_t, int64_t*, int32_t*,
                      hipStream_t);
int zk_expand_acl(const uint8_t*, const int64_t*, const int32_t*,
                  const int64_t*, int64_t, int32_t*, int64_t*, int32_t*,
                  int64_t*, int32_t*, hipStream_t);
int zk_decode_requests(const uint8_t*, const int64_t*, const int32_t*,
                       const int64_t*, int64_t, const ZkReqOut*, hipStream_t);
int zk_decode_connect_responses(const uint8_t*, const int64_t*,
                                const int32_t*, int64_t, int32_t*, int32_t*,
                                int64_t*, int64_t*, int32_t*, int32_t*,
                                hipStream_t);
int zk_tree_fill(const ZkTree*, int64_t, int64_t, const int32_t*, int64_t,
                 hipStream_t);
int zk_tree_build(const ZkTree*, int64_t, int64_t, hipStream_t);
// every hash entry back to empty (before a rebuild)
int zk_tree_ht_reset(const ZkTree*, hipStream_t);
// the free ring's pending entries rebuilt in node order (between batches)
int64_t zk_tree_free_workspace(int64_t cap);
int zk_tree_free_compact(const ZkTree*, int64_t*, hipStream_t);
int zk_tree_serve(const ZkTree*, const uint8_t*, const ZkReqOut*,
                  const int64_t*, int64_t, const ZkServeOut*, int64_t,
                  int64_t, hipStream_t);
// (last int32: read_only; the finish is zk_tree_finish_scan's)
int zk_tree_serve_frames(const ZkTree*, const uint8_t*, const int64_t*,
                         const int32_t*, const int64_t*, int64_t,
                         const ZkServeOut*, int64_t, int64_t, int32_t,
                         int64_t*, int32_t, hipStream_t);
// zk_tree_serve_frames after a rows-deferred scan of the request stream
int zk_tree_serve_tiles(const ZkTree*, const ZkFrameTiles*, int64_t*,
                        int32_t*, const int64_t*, int64_t, const ZkServeOut*,
                        int64_t, int64_t, int32_t, int64_t*, int32_t,
                        hipStream_t);
int zk_tree_finish_scan(const ZkTree*, const int64_t*, int64_t, int32_t,
                        int64_t, int64_t*, int64_t*, hipStream_t);
int zk_tree_serve_ordered(const ZkTree*, const uint8_t*, const ZkReqOut*,
                          const int64_t*, int64_t, const ZkServeOut*, int64_t,
                          int64_t, uint8_t*, int64_t, int32_t, int64_t,
                          int64_t, int32_t, int64_t*, hipStream_t);
int zk_watch_events(const int32_t*, const int32_t*, const int64_t*, int64_t,
                    const int64_t*, int64_t*, int64_t, int32_t*, int32_t*,
                    int64_t*, int32_t*, int64_t*, hipStream_t);
int zk_watch_resume(const ZkTree*, const uint8_t*, const int64_t*,
                    const int32_t*, const int64_t*, int64_t, int32_t,
                    int64_t*, int64_t, int64_t, int32_t*, int64_t*, int32_t*,
                    int64_t*, hipStream_t);
int64_t zk_tree_order_workspace(int64_t);
int64_t zk_tree_order_stats_offset(int64_t);
int zk_tree_expire(const ZkTree*, int64_t, int64_t, unsigned long long*,
                   int64_t*, int64_t, hipStream_t);
// The watch table's maintenance (tree_watch.hip): clear watcher slot wslot's
// bit from every mask; insert every entry of an old table (keys + tags,
// masks, hmask) that has a non-zero mask into the tree's (zeroed) table.
int zk_watch_drop(const ZkTree*, int32_t, hipStream_t);
int zk_watch_rebuild(const ZkTree*, const int64_t*, const int64_t*, int64_t,
                     hipStream_t);
// SEQUENTIAL numbers of a batch in stream order (tree_seq.hip): bytes of
// the workspace for ncap requests, the prefix of it that must be zero when
// it is first used (the kernels leave it zero), and the ordering itself
// (writes seqno[ncap]; bumps each parent's cversion once per batch).
int64_t zk_tree_seq_workspace(int64_t ncap);
int64_t zk_tree_seq_zeroed(int64_t ncap);
void zk_tree_seq_debug(int64_t* buf);
// tree_expire_k's phase clocks: 4 int32 per node of the expiries that follow
// (the buffer covers the tree's node capacity; nullptr turns them off)
void zk_tree_expire_debug(int32_t* buf);
int zk_tree_seq_order(const ZkTree*, const uint8_t*, const int64_t*,
                      const int32_t*, const int64_t*, int64_t, uint8_t*,
                      int64_t, int64_t*, hipStream_t);
// order-independent digest of the live nodes: out[0] = sum of per-node
// hashes (path, czxid, mzxid, version, cversion, numChildren, owner, pzxid,
// data), out[1] = live nodes, out[2] = hash entries in use (live +
// tombstones), out[3] = tombstones
int zk_tree_digest(const ZkTree*, unsigned long long*, hipStream_t);
// GET_CHILDREN / GET_CHILDREN2 batches from the tree (tree_list.hip):
// bytes of the workspace for ncap requests, and the serve itself (frames,
// count, ncap, watcher slot, max reply frame, want[node cap] int32 idling at
// 0x7fffffff, workspace + bytes, out + capacity, rec_off[ncap], total, err,
// terminate)
int64_t zk_tree_list_workspace(int64_t ncap);
int zk_tree_list(const ZkTree*, const uint8_t*, const int64_t*,
                 const int32_t*, const int64_t*, int64_t, int32_t, int64_t,
                 int32_t*, uint8_t*, int64_t, uint8_t*, int64_t, int64_t*,
                 int64_t*, int32_t*, int32_t, hipStream_t);
// The ACL path (tree_acl.hip): bytes of the workspace for ncap requests
// (both passes share it); the record pass after a serve (frames, count, ncap,
// the serve's r_op / r_err / r_node, workspace + bytes); the GET_ACL serve
// (frames, count, ncap, workspace + bytes, out + capacity, rec_off[ncap],
// total, err, terminate), with zk_tree_list's conventions
int64_t zk_tree_acl_workspace(int64_t ncap);
int zk_tree_acl_record(const ZkAclTable*, const uint8_t*, const int64_t*,
                       const int32_t*, const int64_t*, int64_t,
                       const int32_t*, const int32_t*, const int64_t*,
                       uint8_t*, int64_t, hipStream_t);
int zk_tree_acl_get(const ZkTree*, const ZkAclTable*, const uint8_t*,
                    const int64_t*, const int32_t*, const int64_t*, int64_t,
                    uint8_t*, int64_t, uint8_t*, int64_t, int64_t*, int64_t*,
                    int32_t*, int32_t, hipStream_t);
// Mixed batches (tree_mix.hip).  The split: workspace bytes for ncap frames;
// (rx, frames, count, ncap, has_acl, cls[ncap], sub[ncap], foff_c[3][ncap],
// flen_c[3][ncap], counts[3], workspace + bytes).  The merge: workspace bytes;
// (cls, sub, count, counts, ncap, then per class c of 3 the engine's stream,
// its buffer's bytes, rec_off_c, total_c, err_c, workspace + bytes, out +
// capacity, rec_off[ncap], total, err, terminate), with zk_tree_list's
// conventions.  zk_tree_mix_small / _wave: the copy's tier bounds (bytes).
int64_t zk_tree_mix_small(void);
int64_t zk_tree_mix_wave(void);
int64_t zk_tree_mix_split_workspace(int64_t ncap);
int zk_tree_mix_split(const uint8_t*, const int64_t*, const int32_t*,
                      const int64_t*, int64_t, int32_t, int32_t*, int32_t*,
                      int64_t*, int32_t*, int64_t*, uint8_t*, int64_t,
                      hipStream_t);
// zk_tree_mix_split under the second rule (zk_mix.h mix_class_setacl): opcode
// 7 goes to the ACL engine's class on a tree with an ACL table.
int zk_tree_mix_split_setacl(const uint8_t*, const int64_t*, const int32_t*,
                             const int64_t*, int64_t, int32_t, int32_t*,
                             int32_t*, int64_t*, int32_t*, int64_t*, uint8_t*,
                             int64_t, hipStream_t);
int64_t zk_tree_mix_merge_workspace(int64_t ncap);
int zk_tree_mix_merge(const int32_t*, const int32_t*, const int64_t*,
                      const int64_t*, int64_t, const uint8_t* const*,
                      const int64_t*, const int64_t* const*,
                      const int64_t* const*, const int32_t* const*, uint8_t*,
                      int64_t, uint8_t*, int64_t, int64_t*, int64_t*, int32_t*,
                      int32_t, hipStream_t);
// The tree image (tree_snap.hip; layout and outcome codes: zk_snap.h).  a:
// the tree's ACL table or null.  Snapshot: workspace bytes for a node
// capacity; zk_tree_snap_size sizes the image on ws (total[0] = image bytes,
// total[1] = records), zk_tree_snap_write then writes it into out[0, out_cap)
// (status[0] = SNAP_OK or SNAP_NO_ROOM, status[1] = -1).  Load: workspace
// bytes for n records; (image + bytes, n as the host read it, data capacity,
// workspace + bytes, status[2] = SNAP_* and the record index) into a fresh,
// empty tree.  None makes a host read.
int64_t zk_tree_snap_workspace(int64_t cap);
int64_t zk_tree_load_workspace(int64_t n);
int zk_tree_snap_size(const ZkTree*, const ZkAclTable*, uint8_t*, int64_t,
                      int64_t*, hipStream_t);
int zk_tree_snap_write(const ZkTree*, const ZkAclTable*, uint8_t*, int64_t,
                       uint8_t*, int64_t, int64_t*, hipStream_t);
int zk_tree_load(const ZkTree*, const ZkAclTable*, const uint8_t*, int64_t,
                 int64_t, int32_t, uint8_t*, int64_t, int64_t*, hipStream_t);
int zk_bench_gen_get(int64_t, uint64_t, int64_t, int64_t, int32_t,
                     const int64_t*, int64_t*, int32_t*, int64_t*, int32_t*,
                     const int64_t*, int64_t*, int64_t*, hipStream_t);
int zk_bench_xids(int64_t, const int64_t*, int32_t*, hipStream_t);
int zk_bench_storm_hs(int32_t, int32_t, int32_t, const int32_t*,
                      const int64_t*, const int32_t*, const int32_t*,
                      const int64_t*, const uint8_t*, const int64_t*,
                      int64_t*, uint8_t*, bool*, hipStream_t);
int zk_bench_check_writes(int64_t, const int32_t*, const int32_t*,
                          const int32_t*, const int32_t*, const int32_t*,
                          const int32_t*, int32_t, const int64_t*,
                          unsigned long long*, unsigned long long*,
                          hipStream_t);
int zk_bench_check_get(int64_t, const int32_t*, const int32_t*,
                       const int32_t*, const int32_t*, const int64_t*,
                       const int32_t*, const int64_t*, const int32_t*,
                       const int32_t*, unsigned long long*, hipStream_t);
int zk_bench_check_notif(int64_t, int64_t, const uint64_t*, const int64_t*,
                         int64_t, int64_t,
                         const int64_t*, const int32_t*, const uint8_t*,
                         const uint8_t*, const int32_t*, const int32_t*,
                         const int32_t*, const int32_t*, const int32_t*,
                         const int64_t*, const int32_t*, unsigned long long*,
                         hipStream_t);
int64_t zk_route_workspace(int64_t n, int32_t world);
int zk_route_requests(int64_t, int32_t, int32_t, const int64_t*,
                      const int32_t*, const uint8_t*, const int64_t*,
                      const int32_t*, int32_t*, int64_t*, int32_t*, int64_t*,
                      int32_t*, int64_t*, int64_t*, hipStream_t);
int zk_seg_pack(const uint8_t*, int64_t, const int64_t*, const int64_t*,
                int64_t, const int64_t*, const int64_t*, int32_t, int32_t,
                int64_t, uint8_t*, unsigned long long*, uint8_t*, int32_t,
                hipStream_t);
int zk_seg_unpack(const uint8_t*, int32_t, int32_t, int64_t, uint8_t*,
                  int64_t*, int64_t*, unsigned long long*, const uint8_t*,
                  int32_t, hipStream_t);
int zk_session_connect(const uint8_t*, const int64_t*, const int32_t*,
                       const int64_t*, int64_t, const ZkSessionTable*,
                       int64_t, uint64_t, int32_t, int32_t, const int64_t*,
                       uint8_t*, int64_t*, int32_t*, hipStream_t);
int zk_session_close(const ZkSessionTable*, const int64_t*, int64_t,
                     int64_t, hipStream_t);
int zk_session_install(const ZkSessionTable*, const int64_t*, int64_t,
                       int64_t, hipStream_t);
int zk_scan_small_i64(const int64_t*, int64_t*, int64_t, int64_t*,
                      hipStream_t);
// Session batches (tree_sess.hip; the rule: zk_sess.h).  zk_sess_assign:
// (frames off / len, count, ncap, starts[S + 1], sessions[S], S, the session
// table or null, its server id) -> f_seg[ncap], first[S + 1], seg_state[S],
// bad[2].  The serves take (..., fired, the segment table: ZkSegs) in place
// of one session and one watcher slot; the ordered one also the deferral's
// tables (ZkOrdClip; its seg_c[0] is then the table's f_seg) or null: a rank
// the passes cannot reach is refused.  zk_sess_ranges:
// (first, S, the reply encode's rec_off / count / ncap / total / err) ->
// rep_off[S + 1], and with slot_first (the grouped notification encode's
// rec_off / count / ecap / total / err) slot_off[65].  zk_sess_group_events:
// int64 words of its workspace; (ev_slot / type / poff / plen, ev_total,
// ecap, workspace) -> the records in slot-major order and slot_first[65].
int zk_sess_assign(const int64_t*, const int32_t*, const int64_t*, int64_t,
                   const int64_t*, const int64_t*, int64_t,
                   const ZkSessionTable*, int64_t, int32_t*, int64_t*,
                   int32_t*, int64_t*, hipStream_t);
int zk_tree_serve_frames_sessions(const ZkTree*, const uint8_t*,
                                  const int64_t*, const int32_t*,
                                  const int64_t*, int64_t, const ZkServeOut*,
                                  int64_t, int64_t*, const ZkSegs*,
                                  hipStream_t);
int zk_tree_serve_ordered_sessions(const ZkTree*, const uint8_t*,
                                   const ZkReqOut*, const int64_t*, int64_t,
                                   const ZkServeOut*, int64_t, uint8_t*,
                                   int64_t, int32_t, int64_t, int64_t,
                                   int64_t*, const ZkSegs*, const ZkOrdClip*,
                                   hipStream_t);
int zk_sess_ranges(const int64_t*, int64_t, const int64_t*, const int64_t*,
                   int64_t, const int64_t*, const int32_t*, int64_t*,
                   const int64_t*, const int64_t*, const int64_t*, int64_t,
                   const int64_t*, const int32_t*, int64_t*, hipStream_t);
int64_t zk_sess_group_workspace(int64_t ecap);
int zk_sess_group_events(const int32_t*, const int32_t*, const int64_t*,
                         const int32_t*, const int64_t*, int64_t, int64_t*,
                         int32_t*, int32_t*, int64_t*, int32_t*, int64_t*,
                         hipStream_t);
// Session batches of any op mix.  zk_sess_split_segments: (f_seg, the
// split's cls / sub, count, ncap) -> f_seg_c0 / c1 / c2 [ncap], each class's
// frame -> segment.  zk_tree_list_sessions / zk_tree_acl_get_sessions:
// zk_tree_list / zk_tree_acl_get with the segment table (ZkSegs; f_seg: the
// class's) after ncap, in place of the watcher slot.
int zk_sess_split_segments(const int32_t*, const int32_t*, const int32_t*,
                           const int64_t*, int64_t, int32_t*, int32_t*,
                           int32_t*, hipStream_t);
int zk_tree_list_sessions(const ZkTree*, const uint8_t*, const int64_t*,
                          const int32_t*, const int64_t*, int64_t,
                          const ZkSegs*, int64_t, int32_t*,
                          uint8_t*, int64_t, uint8_t*, int64_t, int64_t*,
                          int64_t*, int32_t*, int32_t, hipStream_t);
int zk_tree_acl_get_sessions(const ZkTree*, const ZkAclTable*,
                             const uint8_t*, const int64_t*, const int32_t*,
                             const int64_t*, int64_t, const ZkSegs*,
                             uint8_t*, int64_t, uint8_t*, int64_t, int64_t*,
                             int64_t*, int32_t*, int32_t, hipStream_t);
// SET_ACL in a session batch (tree_setacl.hip; the rule: zk_setacl.h).
// zk_tree_acl_setacl_sessions: zk_tree_acl_get_sessions with rx's length
// after rx and, after the segment table, the peers' addresses [S] (null: no
// ADMIN check), their identities (null: none), the rounds a node, the claim
// words + their count (all 0x7fffffff between calls), stats[8], and behind
// the ACL engine's workspace the pass's own (zk_tree_setacl_workspace bytes).
int64_t zk_tree_setacl_workspace(int64_t ncap);
int zk_tree_acl_setacl_sessions(const ZkTree*, const ZkAclTable*,
                                const uint8_t*, int64_t, const int64_t*,
                                const int32_t*, const int64_t*, int64_t,
                                const ZkSegs*, const int32_t*,
                                const ZkAuthTable*, int32_t, int32_t*, int64_t,
                                int64_t*, uint8_t*, int64_t, uint8_t*, int64_t,
                                uint8_t*, int64_t, int64_t*, int64_t*,
                                int32_t*, int32_t, hipStream_t);
// The SET_WATCHES catch-up of a session batch (tree_resume.hip; the rules:
// zk_resume.h), after its serve: (tree, rx, its length, frames off / len,
// count, ncap, the segment table, workspace, ecap) -> the
// events in stream order (ev_slot / type / poff / plen [ecap], ev_total[2]),
// grouped by watcher slot (g_* [ecap], slot_first[65]) and stats[8].  The
// workspace: int64 words for (ncap, ecap).
int64_t zk_watch_resume_sessions_workspace(int64_t ncap, int64_t ecap);
int zk_watch_resume_sessions(const ZkTree*, const uint8_t*, int64_t,
                             const int64_t*, const int32_t*, const int64_t*,
                             int64_t, const ZkSegs*, int64_t*, int64_t,
                             int32_t*, int32_t*, int64_t*, int32_t*, int64_t*,
                             int32_t*, int32_t*, int64_t*, int32_t*, int64_t*,
                             int64_t*, hipStream_t);
// Close / expire many sessions in one pass (tree_close.hip; the rules:
// zk_close.h).  zk_close_workspace: int64 words for (frames a batch, sessions
// a list, the tree's node slots); its head is the fired watches' record area
// (zk_tree_expire's rec, cap_frames records).  zk_close_frames, between a
// session batch's serve and its reply encode: (tree, rx, its length, frames
// off / len, count, ncap, the segment table, the serve's r_err, cap_frames,
// node slots, workspace) -> every CLOSE_SESSION frame of a live segment
// answered OK, the closing segments' list and count in the workspace,
// stats[8].  zk_close_sessions: (tree, sids[K], wslots[K]
// or null, K, S, cap_frames, node slots, the session table or null, its
// server id, workspace) -> removed[S] (+= per listed session), stats[8];
// sids null: the list zk_close_frames left.
int64_t zk_close_workspace(int64_t cap_frames, int64_t S, int64_t node_cap);
int zk_close_frames(const ZkTree*, const uint8_t*, int64_t, const int64_t*,
                    const int32_t*, const int64_t*, int64_t, const ZkSegs*,
                    int32_t*, int64_t, int64_t, int64_t*, int64_t*,
                    hipStream_t);
int zk_close_sessions(const ZkTree*, const int64_t*, const int32_t*, int64_t,
                      int64_t, int64_t, int64_t, const ZkSessionTable*,
                      int64_t, int64_t*, unsigned long long*, int64_t*,
                      hipStream_t);
// ACL enforcement around a session batch of any op mix (tree_aclperm.hip; the
// rule: zk_aclperm.h).  zk_aclperm_check, after zk_sess_assign and before the
// split: (tree, ACL table, rx — written —, its length, frames off / len,
// count, ncap, the whole batch's segment table, addrs[S]: each segment's peer
// IPv4 address in host order, 0 none) -> deny[ncap], the denied frames' opcode
// words in rx overwritten, stats[8] += (checked, denied, denied for a lost
// binding).  zk_aclperm_fix, between the serve and its reply encode: (deny,
// the split's cls / sub, the whole batch's count, ncap) -> the serve's r_err
// of a denied frame NO_AUTH, stats[3] += the replies so answered.
int zk_aclperm_check(const ZkTree*, const ZkAclTable*, uint8_t*, int64_t,
                     const int64_t*, const int32_t*, const int64_t*, int64_t,
                     const ZkSegs*, const int32_t*, int32_t*, int64_t*,
                     hipStream_t);
int zk_aclperm_fix(const int32_t*, const int32_t*, const int32_t*,
                   const int64_t*, int64_t, int32_t*, int64_t*, hipStream_t);
// AUTH with digest identities around a session batch (tree_auth.hip; the rule:
// zk_auth.h).  zk_auth_frames, after zk_sess_assign and before the ACL check:
// (rx, its length, frames off / len, count, ncap, the whole batch's segment
// table, the identity table of at least as many rows) -> res[ncap] (0 not an
// AUTH frame or a refused segment, 1 stored, 2 AUTH_FAILED), the new
// identities in the table, its stats[0..3] += (ok, failed, full, known).
// zk_aclperm_check_auth: zk_aclperm_check where a `digest` entry grants to a
// row that holds its id.  zk_auth_fix, where zk_aclperm_fix runs: (res, the
// split's cls / sub, the whole batch's count, ncap) -> the serve's r_err of an
// AUTH frame OK or AUTH_FAILED, stats[4], stats[5] += the replies so answered.
int64_t zk_auth_row_bytes(void);
int zk_auth_frames(const uint8_t*, int64_t, const int64_t*, const int32_t*,
                   const int64_t*, int64_t, const ZkSegs*, const ZkAuthTable*,
                   int32_t*, hipStream_t);
int zk_aclperm_check_auth(const ZkTree*, const ZkAclTable*, uint8_t*, int64_t,
                          const int64_t*, const int32_t*, const int64_t*,
                          int64_t, const ZkSegs*, const int32_t*,
                          const ZkAuthTable*, int32_t*, int64_t*, hipStream_t);
int zk_auth_fix(const int32_t*, const int32_t*, const int32_t*, const int64_t*,
                int64_t, int32_t*, int64_t*, hipStream_t);
// The front end's I/O staging (front.hip; the rules: zk_front.h).
// zk_front_chunk: bytes of the cut's staged window.  zk_front_cut: (raw, n,
// raw_starts[S + 1], S, quota, max_packet) -> take[S], nfr[S], flag[S],
// fault[1].  zk_front_gather: (streams[4] and caps[4] on the host, p_stream[P]
// or null, p_src[P], the scanned p_off[P + 1], P, dst, its capacity) -> the
// pieces packed into dst, over[1].  zk_front_tx_pieces: (rep_off[S + 1] or
// null, wslots[S], slot_off[3] on the host — each [65] or null —, the batch's
// err or null, caps[4] on the host, S, owner[64]) -> p_stream / p_src / p_len
// [4 S], stats[8].
int64_t zk_front_chunk(void);
int zk_front_cut(const uint8_t*, int64_t, const int64_t*, int64_t, int64_t,
                 int64_t, int64_t*, int32_t*, int32_t*, int64_t*, hipStream_t);
int zk_front_gather(const uint8_t* const*, const int64_t*, const int32_t*,
                    const int64_t*, const int64_t*, int64_t, uint8_t*, int64_t,
                    int64_t*, hipStream_t);
int zk_front_tx_pieces(const int64_t*, const int32_t*, const int64_t* const*,
                       const int32_t*, const int64_t*, int64_t, int64_t*,
                       int32_t*, int64_t*, int64_t*, int64_t*, hipStream_t);
// The front end in front of the ordered session serve.  zk_front_cut_mode:
// zk_front_cut with (mode, has_acl) after max_packet and nwr[S] after flag;
// mode 0 is zk_front_cut (nwr null), mode 1 the ordered rule
// (zk_front.h front_walk_ordered).  zk_front_tx_pieces_end: zk_front_tx_pieces
// with rep_end[S] (or null) after rep_off.
int zk_front_cut_mode(const uint8_t*, int64_t, const int64_t*, int64_t,
                      int64_t, int64_t, int32_t, int32_t, int64_t*, int32_t*,
                      int32_t*, int32_t*, int64_t*, hipStream_t);
int zk_front_tx_pieces_end(const int64_t*, const int64_t*, const int32_t*,
                           const int64_t* const*, const int32_t*,
                           const int64_t*, int64_t, int64_t*, int32_t*,
                           int64_t*, int64_t*, int64_t*, hipStream_t);
// Deferral in the ordered session serve (ZkOrdClip above) apart from the
// serve.  zk_order_clip: the stage alone over (rank[ncap], passes, the tables
// — bad null —, ncap).  zk_order_clip_ranges: (clipf, rep_off[S + 1], the
// merged rec_off, the frames' off, starts[S + 1], count, ncap, S) ->
// rep_end[S], used[S].
int zk_order_clip(const uint8_t*, int32_t, const ZkOrdClip*, int64_t,
                  hipStream_t);
int zk_order_clip_ranges(const int64_t*, const int64_t*, const int64_t*,
                         const int64_t*, const int64_t*, const int64_t*,
                         int64_t, int64_t, int64_t*, int64_t*, hipStream_t);
}  // extern "C"

// Layout pins (LP64 on both sides: pointers and int64_t are 8 bytes).
static_assert(sizeof(void*) == 8, "LP64 only");
static_assert(sizeof(ZkReqBatch) == 13 * 8, "ZkReqBatch layout");
static_assert(sizeof(ZkNodeStore) == 5 * 8, "ZkNodeStore layout");
static_assert(sizeof(ZkRespBatch) == 10 * 8, "ZkRespBatch layout");
static_assert(sizeof(ZkReplyOut) == 12 * 8, "ZkReplyOut layout");
static_assert(sizeof(ZkReqOut) == 12 * 8, "ZkReqOut layout");
static_assert(sizeof(ZkServeOut) == 10 * 8, "ZkServeOut layout");
static_assert(sizeof(ZkSegs) == 6 * 8, "ZkSegs layout");
static_assert(sizeof(ZkOrdClip) == 11 * 8, "ZkOrdClip layout");
static_assert(sizeof(ZkSessionTable) == 7 * 8, "ZkSessionTable layout");
static_assert(sizeof(ZkAclTable) == 8 * 8, "ZkAclTable layout");
static_assert(offsetof(ZkAclTable, arena) == 2 * 8, "ZkAclTable.arena");
static_assert(offsetof(ZkAclTable, hmask) == 6 * 8, "ZkAclTable.hmask");
static_assert(sizeof(ZkTree) == 27 * 8, "ZkTree layout");
static_assert(sizeof(ZkFrameTiles) == 14 * 8, "ZkFrameTiles layout");
static_assert(offsetof(ZkFrameTiles, fblk) == 11 * 8, "ZkFrameTiles.fblk");
static_assert(offsetof(ZkTree, store) == 9 * 8, "ZkTree.store");
static_assert(offsetof(ZkTree, free_list) == 14 * 8, "ZkTree.free_list");
static_assert(offsetof(ZkTree, wt_hmask) == 25 * 8, "ZkTree.wt_hmask");
static_assert(offsetof(ZkRespBatch, slot) == 9 * 8, "ZkRespBatch.slot");
static_assert(offsetof(ZkReplyOut, cap) == 11 * 8, "ZkReplyOut.cap");
static_assert(offsetof(ZkReqOut, rel_zxid) == 10 * 8, "ZkReqOut.rel_zxid");
