"""The HIP batch codec as PyTorch-ROCm operators: ``torch.ops.zkmi.*``.

``zkmi/ops/libzkmi_torch.so`` (csrc/torch/zkmi_ops.cpp) registers the ops
with ``TORCH_LIBRARY(zkmi, ...)``; the kernels themselves live in
``zkmi/ops/libzkmi_hip.so`` (csrc/kernels/*.hip, gfx950), which the op
library links.  Both are compiled in-tree by ``tools/build_native.py``
(called from ``__graft_entry__.build``).  Every op checks dtype, device,
contiguity and lengths of its tensors before a pointer reaches a kernel,
runs on the current HIP stream and raises on a launch error.

On a machine with a GPU a missing library is an error (:func:`lib`
raises); there is no silent CPU fallback for the batch codec.  So is a
kernel library built from other sources than this tree's
(``zkmi/ops/_srchash.py``): its embedded source hash must match.
"""

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libzkmi_torch.so')
HIP_LIB_PATH = os.path.join(_HERE, 'libzkmi_hip.so')

# wire-format node slot layout (csrc/kernels/zk_abi.h)
SLOT_STAT = 0
SLOT_LEN = 72
SLOT_DATA = 76

# session handshake outcomes (csrc/kernels/session.hip SC_*)
SC_NEW, SC_RESUMED, SC_EXPIRED, SC_REFUSED, SC_BAD, SC_FULL = range(6)
CR_RESP_BYTES = 41

# ZkTree counters (csrc/kernels/zk_tree.h TC_*)
TC_NODES, TC_ZXID, TC_PATH_TOP, TC_SLAB_TOP = 0, 1, 2, 3
TC_FREE_HEAD, TC_FREE_TAIL, TC_FREE_PUB, TC_DIRTY = 4, 5, 6, 7
TC_SESS, TC_N = 8, 9
# serve / expire `session` argument: the one in counters[TC_SESS]
SESS_DEV = -2
HT_WORDS = 8     # int64 words per hash entry: key, val, lengths, path head
# watch table (zk_tree.h): counter words behind the masks, the lost-arm one
WT_STATS, WS_LOST = 8, 0

SCAN_SHFL, SCAN_MFMA, SCAN_MFMA_W1, SCAN_MFMA_W4 = 0, 1, 2, 3
SCAN_MFMA_FORCE = 4      # the multi-block MFMA path at any n (tests)

_ops = None


def lib():
    """Load (once) the operator library and return ``torch.ops.zkmi``."""
    global _ops
    if _ops is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'zkmi operator library not built: run `python tools/'
                'build_native.py` (or __graft_entry__.build())')
        check_build()
        torch.ops.load_library(LIB_PATH)
        _ops = torch.ops.zkmi
        # the MFMA byte-plane scan engine (csrc/kernels/scan.hip); the
        # shuffle engine stays selectable (scan_set_mode) for the tests
        _ops.scan_set_mode(SCAN_MFMA)
    return _ops


def built_hash():
    """The source hash embedded in ``libzkmi_hip.so`` (None if absent)."""
    try:
        f = ctypes.CDLL(HIP_LIB_PATH).zkmi_hip_src_hash
    except (OSError, AttributeError):
        return None
    f.restype = ctypes.c_char_p
    return f().decode()


def check_build():
    """Raise unless the kernel library was compiled from this tree's kernel
    sources and flags (``ZKMI_ALLOW_STALE_BUILD=1`` skips the check for
    A/B runs that swap libraries on purpose)."""
    from . import _srchash
    if os.environ.get('ZKMI_ALLOW_STALE_BUILD') == '1':
        return
    want, got = _srchash.hip_hash(), built_hash()
    if got != want:
        raise RuntimeError(
            'zkmi/ops/libzkmi_hip.so was built from other sources (hash %s, '
            'tree %s): run `python tools/build_native.py`' % (got, want))


def set_scan_mode(mode):
    """Select the prefix-scan engine used by every encoder; returns the
    previous mode."""
    return lib().scan_set_mode(mode)


# idle value of the list path's per-node claim words (tree_list.hip LS_NONE)
LIST_IDLE = 0x7fffffff


def tree_list_workspace(ncap):
    """Bytes of the workspace :func:`tree_list` needs for ``ncap`` requests
    (a uint8 tensor; nothing in it needs zeroing)."""
    return lib().tree_list_workspace(int(ncap))


def tree_list(tree, rx, frame_off, frame_len, count, ncap, wslot, max_frame,
              want, ws, out, out_cap, rec_off, total, err, terminate=False):
    """Serve a batch of GET_CHILDREN / GET_CHILDREN2 frames from the HBM
    tree (csrc/kernels/tree_list.hip), on the current stream: the framed
    replies in request order -> ``out[:total]``, their starts ->
    ``rec_off``.  ``want``: int32 per node slot, all :data:`LIST_IDLE`
    between calls (the kernels put it back).  ``err`` 2 and ``total`` 0:
    the stream did not fit ``out_cap``."""
    lib().tree_list(tree, rx, frame_off, frame_len, count, int(ncap),
                    int(wslot), int(max_frame), want, ws, out, int(out_cap),
                    rec_off, total, err, bool(terminate))


# ACL table (csrc/kernels/tree_acl.hip): a lost binding, the counter words
ACL_LOST = -1
AC_TOP, AC_ENT, AC_LOST, AC_OLD_TOP, AC_LIMIT = 0, 1, 2, 3, 4


def acl_hash(raw):
    """Key of the ACL vector ``raw`` (wire bytes) in the intern index: the
    host mirror of csrc/kernels/zk_tree.h path_hash, | 1."""
    m64 = (1 << 64) - 1
    n = len(raw)
    h = 0x9E3779B97F4A7C15 ^ n
    for i in range(0, n, 8):
        w = int.from_bytes(raw[i:i + 8], 'little')
        h = ((h ^ w) * 0xFF51AFD7ED558CCD) & m64
        h ^= h >> 32
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & m64
    h ^= h >> 33
    return h | 1


def tree_acl_workspace(ncap):
    """Bytes of the workspace :func:`tree_acl_record` and
    :func:`tree_acl_get` need for ``ncap`` requests (one uint8 tensor serves
    both; nothing in it needs zeroing)."""
    return lib().tree_acl_workspace(int(ncap))


def tree_acl_record(acl, rx, frame_off, frame_len, count, ncap, r_op, r_err,
                    r_node, ws):
    """After a serve, on its stream: intern the ACL vector of every
    successful CREATE of the batch (``r_op`` / ``r_err`` / ``r_node``: the
    serve's reply descriptors) in the table ``acl`` (``GpuTree.acl``) and
    bind it to the created node.  Two launches, no host read."""
    lib().tree_acl_record(acl, rx, frame_off, frame_len, count, int(ncap),
                          r_op, r_err, r_node, ws)


def tree_acl_get(tree, acl, rx, frame_off, frame_len, count, ncap, ws, out,
                 out_cap, rec_off, total, err, terminate=False):
    """Serve a batch of GET_ACL frames from the HBM tree and its ACL table
    (csrc/kernels/tree_acl.hip), on the current stream: the framed replies
    in request order -> ``out[:total]``, their starts -> ``rec_off``.
    ``err`` 2 and ``total`` 0: the stream did not fit ``out_cap``."""
    lib().tree_acl_get(tree, acl, rx, frame_off, frame_len, count, int(ncap),
                       ws, out, int(out_cap), rec_off, total, err,
                       bool(terminate))


# outcome of an image load / a fixed-buffer snapshot (csrc/kernels/zk_snap.h
# SNAP_*; zkmi/utils/treeimage.py mirrors them)
(SNAP_OK, SNAP_BAD_HEADER, SNAP_BAD_TABLE, SNAP_BAD_RECORD, SNAP_NO_ROOM,
 SNAP_DUP_PATH, SNAP_ORPHAN, SNAP_DIGEST) = range(8)


def tree_snap_workspace(cap):
    """Bytes of the workspace :func:`tree_snap_size` / :func:`tree_snap_write`
    need for a tree of ``cap`` node slots (a uint8 tensor; nothing in it
    needs zeroing)."""
    return lib().tree_snap_workspace(int(cap))


def tree_load_workspace(n):
    """Bytes of the workspace :func:`tree_load` needs for an image of ``n``
    records (a uint8 tensor; nothing in it needs zeroing)."""
    return lib().tree_load_workspace(int(n))


def tree_snap_size(tree, acl, ws, total):
    """Size the image of the tree's live znodes on ``ws``, on the current
    stream (csrc/kernels/tree_snap.hip): ``total`` (int64 [2]) = image
    bytes, records.  ``acl``: the tree's ACL table (``GpuTree.acl``) or an
    empty list.  No host read."""
    lib().tree_snap_size(tree, list(acl or []), ws, total)


def tree_snap_write(tree, acl, ws, out, out_cap, status):
    """Write the image :func:`tree_snap_size` just sized on ``ws`` into
    ``out[:out_cap]`` (16-byte aligned).  ``status`` (int64 [2]):
    :data:`SNAP_OK`, or :data:`SNAP_NO_ROOM` when the image does not fit —
    nothing is written then.  No host read."""
    lib().tree_snap_write(tree, list(acl or []), ws, out, int(out_cap),
                          status)


def tree_load(tree, acl, image, image_len, n, data_cap, ws, status):
    """Load ``image[:image_len]`` (``n`` records by the host's reading of
    its header; the device checks it) into the fresh, empty ``tree``.
    ``status`` (int64 [2]): the ``SNAP_*`` outcome and the record index it
    was found at (-1: none).  A refused image is a normal outcome; the tree
    is then unusable.  No host read."""
    lib().tree_load(tree, list(acl or []), image, int(image_len), int(n),
                    int(data_cap), ws, status)


# engine classes of a mixed batch, in engine order (csrc/kernels/zk_mix.h):
# the fused serve, the GET_ACL path, the list path
MIX_A, MIX_C, MIX_L = 0, 1, 2


def tree_mix_bounds():
    """(small, wave): the tier bounds of the merge's copy kernels in bytes
    (csrc/kernels/tree_mix.hip MIX_SMALL / MIX_WAVE)."""
    return lib().tree_mix_small(), lib().tree_mix_wave()


def tree_mix_split_workspace(ncap):
    """Bytes of the workspace :func:`tree_mix_split` needs for ``ncap``
    frames (a uint8 tensor; nothing in it needs zeroing)."""
    return lib().tree_mix_split_workspace(int(ncap))


def tree_mix_merge_workspace(ncap):
    """Bytes of the workspace :func:`tree_mix_merge` needs for ``ncap``
    requests (a uint8 tensor; nothing in it needs zeroing)."""
    return lib().tree_mix_merge_workspace(int(ncap))


def tree_mix_split(rx, frame_off, frame_len, count, ncap, has_acl, cls, sub,
                   frame_off_c, frame_len_c, counts, ws):
    """Split a batch's frame table by engine class, on the current stream
    (csrc/kernels/tree_mix.hip): ``cls`` / ``sub`` (int32 [ncap]: class and
    index inside the class; -1 / 0 past ``count``), the compacted tables
    ``frame_off_c`` (int64) / ``frame_len_c`` (int32), both [3 * ncap] with
    class c's at ``c * ncap``, and ``counts`` (int64 [3]).  Stable: request
    order is kept inside a class.  No host read."""
    lib().tree_mix_split(rx, frame_off, frame_len, count, int(ncap),
                         bool(has_acl), cls, sub, frame_off_c, frame_len_c,
                         counts, ws)


def tree_mix_split_setacl(rx, frame_off, frame_len, count, ncap, has_acl, cls,
                          sub, frame_off_c, frame_len_c, counts, ws):
    """:func:`tree_mix_split` for a caller that serves SET_ACL: a frame with
    opcode 7 is of the ACL engine's class (1) on a tree with an ACL table
    (zk_mix.h mix_class_setacl); every other frame as there.  The same
    launches."""
    lib().tree_mix_split_setacl(rx, frame_off, frame_len, count, int(ncap),
                                bool(has_acl), cls, sub, frame_off_c,
                                frame_len_c, counts, ws)


def tree_mix_merge(cls, sub, count, counts, ncap, streams, rec_offs, totals,
                   errs, out, out_cap, rec_off, total, err, ws,
                   terminate=False):
    """Merge the three engines' reply streams into request order, on the
    current stream: request i takes reply ``sub[i]`` of stream ``cls[i]``
    (``streams`` / ``rec_offs`` / ``totals`` / ``errs``: a tensor per class)
    -> ``out[:total]``, the starts -> ``rec_off``.  An engine's non-zero
    ``err`` is the merged one (class 0 first), else ``err`` 2 when the stream
    does not fit ``out_cap``; then ``total`` is 0 and nothing is written."""
    lib().tree_mix_merge(cls, sub, count, counts, int(ncap), list(streams),
                         list(rec_offs), list(totals), list(errs), out,
                         int(out_cap), rec_off, total, err, bool(terminate),
                         ws)


# session batches (csrc/kernels/tree_sess.hip; the rule: zk_sess.h)
SEG_SERVE, SEG_EXPIRED = 0, 1       # seg_state values
SESS_SLOTS = 64                     # watcher slots of a server


def sess_assign(frame_off, frame_len, count, ncap, starts, sessions, f_seg,
                first, seg_state, bad, table=None, server_id=0, span=0):
    """A session batch's frames -> segments, on the current stream:
    ``f_seg`` (int32 [ncap], written for the batch's frames), ``first``
    (int64 [S + 1]: each segment's first frame), ``seg_state`` (int32 [S]:
    :data:`SEG_SERVE`, or :data:`SEG_EXPIRED` when ``table`` — a session
    table's tensors — does not hold the segment's session alive) and ``bad``
    (int64 [2]: torn frames + faults of the table, the first bad segment or
    -1).  Two launches, no host read."""
    lib().sess_assign(frame_off, frame_len, count, int(ncap), starts,
                      sessions, list(table or []), int(server_id), int(span),
                      f_seg, first, seg_state, bad)


def tree_serve_frames_sessions(tree, rx, frame_off, frame_len, count, ncap,
                               out, now_ms, fired, seqno, segs):
    """``tree_serve_frames`` for a session batch: every frame is served for
    its segment's session and watcher slot.  ``segs``: the segment table,
    ``[f_seg, sessions, wslots, seg_state, bad]`` — :func:`sess_assign`'s
    outputs and the caller's sessions / wslots (int64 / int32 [S]); every op
    of a session batch takes it in this form.  A batch with ``bad[0] != 0``
    is refused SYSTEMERROR, a segment with state :data:`SEG_EXPIRED`
    SESSION_EXPIRED.  ``tree_finish_scan`` follows."""
    lib().tree_serve_frames_sessions(tree, rx, frame_off, frame_len, count,
                                     int(ncap), out, int(now_ms), fired,
                                     seqno, list(segs))


def tree_serve_ordered_sessions(tree, rx, requests, count, ncap, out, now_ms,
                                ws, passes, scratch, fired, seqno, segs,
                                clip=None):
    """``tree_serve_ordered`` for a session batch: requests on one path are
    applied in stream order whichever segments they come from.

    ``clip`` (``[cls, sub, count_all, f_seg_all, seg_c0, seg_c1, seg_c2,
    clipf, deferred]``): the serve's class of a session batch of any op mix
    (``requests`` / ``count``: the class's decoded frames; ``segs[0]`` their
    segments, the same tensor as ``seg_c0``), with deferral in place of the
    rank refusal (csrc/kernels/tree_order.hip ord_clip_*; the rules:
    zk_order_clip.h).  Between the ranking and the first serve pass, three
    launches over the WHOLE batch's tables (``cls`` / ``sub``: the split's,
    ``count_all``, ``f_seg_all``: :func:`sess_assign`'s, ``seg_c*``: the three
    classes' segment tables): a frame of the serve's class whose rank is >=
    ``passes``, and every later frame of its segment, gets segment -1 in
    ``f_seg_all`` and ``seg_c*`` — every engine, the catch-up and the close
    pass refuse it without effect.  ``clipf`` (int64 [S]): the first deferred
    whole-batch frame of each segment (``ncap``: none); ``deferred`` (int64
    [1]): the frames deferred.  No host read."""
    lib().tree_serve_ordered_sessions(tree, rx, requests, count, int(ncap),
                                      out, int(now_ms), ws, int(passes),
                                      scratch, fired, seqno, list(segs),
                                      None if clip is None else list(clip))


def order_clip(rank, passes, ncap, clip):
    """The deferral stage of :func:`tree_serve_ordered_sessions` alone
    (``clip`` as there), over a rank table of the caller's (uint8 [ncap],
    indexed by the serve class's ``sub``; the low 7 bits are the rank)."""
    lib().order_clip(rank, int(passes), int(ncap), list(clip))


def order_clip_ranges(clipf, rep_off, rec_off, frame_off, starts, count_all,
                      ncap, rep_end, used):
    """After the merge and :func:`sess_ranges` of a batch served with
    deferral: ``rep_end`` (int64 [S]) — connection s's replies are
    ``out[rep_off[s]:rep_end[s]]``, the placeholders of its deferred frames
    lie behind — and ``used`` (int64 [S]), the request bytes of segment s that
    were consumed (all of them for a segment that was not clipped).
    ``rec_off``: the merged reply starts; ``frame_off``: the whole batch's
    frame table.  One launch, no host read."""
    lib().order_clip_ranges(clipf, rep_off, rec_off, frame_off, starts,
                            count_all, int(ncap), rep_end, used)


def sess_ranges(first, rec_off, count, ncap, total, err, rep_off,
                slot_first=None, ev_rec_off=None, ev_count=None,
                ev_bytes=None, ev_err=None, slot_off=None):
    """After the reply encode: ``rep_off`` (int64 [S + 1]) — connection s's
    replies are ``out[rep_off[s]:rep_off[s + 1]]``.  With ``slot_first``
    (after the grouped notification encode): ``slot_off`` (int64 [65])
    likewise per watcher slot.  One launch."""
    lib().sess_ranges(first, rec_off, count, int(ncap), total, err, rep_off,
                      slot_first, ev_rec_off, ev_count, ev_bytes, ev_err,
                      slot_off)


def sess_group_workspace(ecap):
    """int64 words of the workspace :func:`sess_group_events` needs for
    ``ecap`` events (nothing in it needs zeroing)."""
    return lib().sess_group_workspace(int(ecap))


def sess_group_events(ev_slot, ev_type, ev_poff, ev_plen, ev_total, ws,
                      g_slot, g_type, g_poff, g_plen, slot_first):
    """The ``ev_total[0]`` events ``watch_events`` wrote, grouped by watcher
    slot (stable: request order inside a slot) -> ``g_*``; ``slot_first``
    (int64 [65]): slot w's records are ``[slot_first[w], slot_first[w +
    1])``.  A histogram and a scatter around the device-wide scan, no host
    read."""
    lib().sess_group_events(ev_slot, ev_type, ev_poff, ev_plen, ev_total, ws,
                            g_slot, g_type, g_poff, g_plen, slot_first)


def sess_split_segments(f_seg, cls, sub, count, ncap, f_seg_c):
    """A session batch of any op mix, after :func:`sess_assign` (``f_seg``)
    and :func:`tree_mix_split` (``cls`` / ``sub``) of one frame table:
    ``f_seg_c[cls[i]][sub[i]] = f_seg[i]`` for every frame of the batch, so
    each engine finds a frame's segment beside its compacted frame table.
    ``f_seg_c``: three int32 [ncap] tensors.  One launch, no host read."""
    lib().sess_split_segments(f_seg, cls, sub, count, int(ncap),
                              list(f_seg_c))


def tree_list_sessions(tree, rx, frame_off, frame_len, count, ncap, segs,
                       max_frame, want, ws, out, out_cap, rec_off, total, err,
                       terminate=False):
    """:func:`tree_list` for the list class of a session batch of any op mix
    (``segs``: the segment table with the class's ``f_seg``):
    frame i is served for segment ``f_seg[i]`` (its ``watch=1`` arms the
    child watch of ``wslots[f_seg[i]]``; outside 0..63: none); with
    ``bad[0] != 0`` every frame is refused SYSTEMERROR, a segment with state
    :data:`SEG_EXPIRED` SESSION_EXPIRED, header only and without effect."""
    lib().tree_list_sessions(tree, rx, frame_off, frame_len, count, int(ncap),
                             list(segs), int(max_frame), want, ws, out,
                             int(out_cap), rec_off, total, err,
                             bool(terminate))


def tree_acl_get_sessions(tree, acl, rx, frame_off, frame_len, count, ncap,
                          segs, ws, out, out_cap, rec_off, total, err,
                          terminate=False):
    """:func:`tree_acl_get` for the GET_ACL class of a session batch of any
    op mix; refusals as :func:`tree_list_sessions`."""
    lib().tree_acl_get_sessions(tree, acl, rx, frame_off, frame_len, count,
                                int(ncap), list(segs), ws, out, int(out_cap),
                                rec_off, total, err, bool(terminate))


# SET_ACL in a session batch (csrc/kernels/tree_setacl.hip; the rule:
# zk_setacl.h).  What GpuServer.setacl_stats reports, in the order of the
# kernels' counters, and the idle value of a node's claim word
SETACL_STATS = ('applied', 'bad_version', 'denied', 'invalid', 'unreached',
                'store_full')
SETACL_IDLE = 0x7fffffff


def tree_setacl_workspace(ncap):
    """Bytes of the SET_ACL pass's workspace for ``ncap`` frames (a uint8
    tensor; nothing in it needs zeroing)."""
    return lib().tree_setacl_workspace(int(ncap))


def tree_acl_setacl_sessions(tree, acl, rx, frame_off, frame_len, count, ncap,
                             segs, addrs, auth, passes, claim, stats, ws, sws,
                             out, out_cap, rec_off, total, err,
                             terminate=False):
    """:func:`tree_acl_get_sessions` for a class that carries SET_ACL frames
    (:func:`tree_mix_split_setacl`): the SET_ACL pass first — judge, intern,
    ``passes`` rounds a node —, then GET_ACL and SET_ACL replies in one
    stream in request order.  ``addrs`` (int32 [S]; None: ADMIN is not
    checked), ``auth`` (the identity table's tensors or None), ``claim``
    (int32, a word a node, all ``SETACL_IDLE`` between calls), ``stats``
    (int64 [8], accumulated, ``SETACL_STATS``), ``sws``
    (:func:`tree_setacl_workspace` bytes).  No host read."""
    lib().tree_acl_setacl_sessions(
        tree, list(acl), rx, frame_off, frame_len, count, int(ncap),
        list(segs), [] if addrs is None else [addrs],
        [] if auth is None else list(auth), int(passes), claim, stats, ws,
        sws, out, int(out_cap), rec_off, total, err, bool(terminate))


# the SET_WATCHES catch-up of a session batch (csrc/kernels/tree_resume.hip;
# the rules: zk_resume.h)
RESUME_CHUNK = 1024     # bytes of a frame staged through LDS at a time: chunk
                        # c of a frame covers rx[c0 + c * RESUME_CHUNK, ...),
                        # c0 = the list start (frame body + 16) rounded down
                        # to 16 (rx itself 16-aligned); zk_resume.h RS_CHUNK
RESUME_STATS = ('events', 'events_written', 'rearmed', 'listed', 'dropped',
                'no_slot')


def watch_resume_sessions_workspace(ncap, ecap):
    """int64 words of :func:`watch_resume_sessions`' workspace for ``ncap``
    frames and ``ecap`` listed paths (nothing in it needs zeroing)."""
    return lib().watch_resume_sessions_workspace(int(ncap), int(ecap))


def watch_resume_sessions(tree, rx, frame_off, frame_len, count, ncap, segs,
                          ws, ev, ev_total, grouped, slot_first, stats):
    """The SET_WATCHES catch-up of a session batch, after its serve and on
    the current stream: every SET_WATCHES frame of the frame table is caught
    up for watcher slot ``wslots[f_seg[i]]`` against the tree as it is now.
    ``ev`` and ``grouped``: [slot int32, type int32, path_off int64, path_len
    int32], each ``ecap`` long (path offsets into ``rx``) — the events in
    stream order and grouped by watcher slot (``slot_first`` int64 [65], as
    :func:`sess_group_events`); ``ev_total`` int64 [2] (written, all);
    ``stats`` int64 [8], :data:`RESUME_STATS` in order.  Nothing is caught
    up when ``bad[0] != 0``, for a segment with state :data:`SEG_EXPIRED` or
    outside the table, for a watcher slot outside 0..63, or for a frame that
    is not a well-formed SET_WATCHES.  No host read."""
    lib().watch_resume_sessions(tree, rx, frame_off, frame_len, count,
                                int(ncap), list(segs), ws, list(ev), ev_total,
                                list(grouped), slot_first, stats)


# close / expire many sessions in one pass (csrc/kernels/tree_close.hip; the
# rules: zk_close.h).  What GpuServer.close_stats reports, in order: the
# first three are the passes' own counters (stats[0..2])
CLOSE_STATS = ('frames', 'sessions', 'removed', 'events_fired',
               'events_written', 'records_dropped', 'encode_err')


def close_workspace(cap_frames, S, node_cap):
    """int64 words of the close passes' workspace for a server of
    ``cap_frames`` frames a batch, lists of up to ``S`` sessions and a tree of
    ``node_cap`` node slots (nothing in it needs zeroing).  Its first ``8 + 5
    * cap_frames`` words are the record area of the watches the removals
    fire, laid out as :meth:`GpuTree.expire`'s ``rec``."""
    return lib().close_workspace(int(cap_frames), int(S), int(node_cap))


def close_frames(tree, rx, frame_off, frame_len, count, ncap, segs, r_err,
                 cap_frames, ws, stats):
    """Between a session batch's serve and its reply encode, on the current
    stream: every CLOSE_SESSION frame of a live segment of a sound table
    (``bad[0] == 0``, state :data:`SEG_SERVE`, a body of 8 bytes or more)
    whose reply the serve left UNIMPLEMENTED is answered OK in ``r_err`` and
    closes its segment.  The closing segments' sessions and watcher slots,
    in segment order, and their number stay in ``ws`` for
    :func:`close_sessions` without ``sids``.  ``stats`` (int64 [8]) is
    zeroed; ``stats[0]`` counts the closing frames.  No host read."""
    lib().close_frames(tree, rx, frame_off, frame_len, count, int(ncap),
                       list(segs), r_err, int(cap_frames), ws, stats)


def close_sessions(tree, sids, wslots, S, cap_frames, ws, removed, stats,
                   table=None, server_id=0, span=0):
    """End the listed sessions in one pass, on the current stream: ``sids``
    (int64 [K], K <= ``S``) with ``wslots`` (int32 [K] or None), or, with
    ``sids`` None, the list :func:`close_frames` left in ``ws``.  The
    ephemerals of session rank k go with zxid base + k + 1 and are counted
    in ``removed[k]`` (accumulated; int64 [K], [S] without ``sids``); the
    zxid counter moves by K.  On a tree with a watch table the listed
    watcher slots' bits are dropped from every mask first, and the watches
    the removals fire are recorded in the head of ``ws``.  ``table``: a
    session table's tensors, whose entries of the listed ids close.
    ``stats`` (int64 [8]): ``[1]`` K, ``[2]`` nodes removed.  ``ws``:
    :func:`close_workspace` of (``cap_frames``, ``S``, the tree's node
    slots).  No host read."""
    lib().close_sessions(tree, sids, wslots, int(S), int(cap_frames),
                         list(table or []), int(server_id), int(span), ws,
                         removed, stats)


# ACL enforcement around a session batch of any op mix
# (csrc/kernels/tree_aclperm.hip; the rule: zk_aclperm.h).  What
# GpuServer.acl_enforce_stats reports, in order (stats[0..2])
ACLPERM_STATS = ('checked', 'denied', 'denied_lost')


def aclperm_check(tree, acl, rx, frame_off, frame_len, count, ncap, segs,
                  addrs, deny, stats):
    """After :func:`sess_assign` and before :func:`tree_mix_split`, on the
    current stream: every frame of the whole batch's frame table whose
    segment is served (``segs``: the whole batch's table), whose body parses
    and whose target exists is checked against the target's ACL in ``acl``
    for its segment's peer ``addrs[f_seg[i]]`` (int32 [S]: the IPv4 address
    as a host-order word, 0 none).  ``deny`` (int32 [ncap]) is written for
    the batch's frames; a denied frame's opcode word in ``rx`` is overwritten
    with an opcode of no request.  ``stats`` (int64 [8]) accumulates
    :data:`ACLPERM_STATS`.  One launch, no host read."""
    lib().aclperm_check(tree, list(acl), rx, frame_off, frame_len, count,
                        int(ncap), list(segs), addrs, deny, stats)


def aclperm_fix(deny, cls, sub, count, ncap, r_err, stats):
    """Between the serve of a session batch's serve class and its reply
    encode: a frame :func:`aclperm_check` denied (``deny``; ``cls`` / ``sub``
    / ``count``: :func:`tree_mix_split`'s over the whole batch) whose reply
    the serve left BAD_ARGUMENTS is answered NO_AUTH in ``r_err`` and counted
    in ``stats[3]``.  One launch, no host read."""
    lib().aclperm_fix(deny, cls, sub, count, int(ncap), r_err, stats)


# AUTH with digest identities around a session batch
# (csrc/kernels/tree_auth.hip; the rule and the record layout: zk_auth.h).
# What GpuServer.auth_stats reports, in order (stats[0..5])
AUTH_STATS = ('ok', 'failed', 'full', 'known', 'answered_ok',
              'answered_failed')
AUTH_K, AUTH_REC, AUTH_ID_MAX, AUTH_MAX = 4, 160, 148, 119
AUTH_FAILED = -115


def auth_row_bytes():
    """Bytes of one row of an identity table's records
    (:data:`AUTH_K` records of :data:`AUTH_REC` bytes)."""
    return lib().auth_row_bytes()


def auth_frames(rx, frame_off, frame_len, count, ncap, segs, auth, res):
    """After :func:`sess_assign` and before the ACL check, on the current
    stream: every AUTH frame (opcode 100) of the whole batch's frame table
    whose segment is served (``segs``: the whole batch's table) is parsed
    and, for the scheme ``digest`` and credentials of at most
    :data:`AUTH_MAX` bytes, its identity ``user:base64(SHA1(credentials))``
    stored in row ``f_seg[i]`` of ``auth`` (``[recs, cnt, stats]``) unless
    the row holds it.  ``res`` (int32 [ncap]) is written for the batch's
    frames: 0 not an AUTH frame or a refused segment, 1 stored or known,
    2 AUTH_FAILED (malformed, another scheme, too long, the row is full).
    ``auth[2]`` accumulates :data:`AUTH_STATS` [0..3].  One launch, no host
    read."""
    lib().auth_frames(rx, frame_off, frame_len, count, int(ncap), list(segs),
                      list(auth), res)


def aclperm_check_auth(tree, acl, rx, frame_off, frame_len, count, ncap, segs,
                       addrs, auth, deny, stats):
    """:func:`aclperm_check` for peers that hold identities: a ``digest``
    entry that carries the bit grants when its id is one of row
    ``f_seg[i]``'s identities in ``auth``.  One launch, no host read."""
    lib().aclperm_check_auth(tree, list(acl), rx, frame_off, frame_len, count,
                             int(ncap), list(segs), addrs, list(auth), deny,
                             stats)


def auth_fix(res, cls, sub, count, ncap, r_err, stats):
    """Where :func:`aclperm_fix` runs: an AUTH frame (``res`` of
    :func:`auth_frames`; ``cls`` / ``sub`` / ``count``:
    :func:`tree_mix_split`'s over the whole batch) whose reply the serve left
    BAD_ARGUMENTS is answered OK (1) or AUTH_FAILED (2) in ``r_err`` and
    counted in ``stats[4]`` / ``stats[5]``.  One launch, no host read."""
    lib().auth_fix(res, cls, sub, count, int(ncap), r_err, stats)


# the front end's TX streams, in the order a connection's pieces are sent
# (csrc/kernels/zk_front.h FS_*), and its assembly counters (FTS_*)
FS_REPLY, FS_RESUME, FS_NOTIF, FS_CLOSE = range(4)
FRONT_PIECES = 4
FRONT_STATS = ('dup_slot',)


def front_chunk():
    """Bytes of :func:`front_cut`'s staged window (csrc/kernels/front.hip
    FC_CHUNK): a word of a segment that straddles a multiple of it is read
    from a window of its own."""
    return lib().front_chunk()


def front_cut(raw, n, raw_starts, quota, max_packet, take, nfr, flag, fault,
              mode=0, has_acl=False, nwr=None):
    """The front end's cut (csrc/kernels/front.hip; the rule: zk_front.h
    front_walk), on the current stream: what every connection has received,
    ``raw[:n]`` with ``raw_starts`` (int64 [S + 1]; segment s is
    ``raw[raw_starts[s]:raw_starts[s + 1]]``, partial trailing frames
    included), cut at a frame boundary.  ``take`` (int64 [S]): the bytes of
    each segment to serve now — whole frames only, at most ``quota`` of them,
    any number of non-write frames or exactly one write frame (CREATE,
    DELETE, SET_DATA, CLOSE_SESSION); ``nfr`` (int32 [S]): the frames in
    them; ``flag`` (int32 [S]): 1 where the walk met a length < 0 or >
    ``max_packet`` (nothing at or after it is taken).  ``fault`` (int64
    [1]): 1 when ``raw_starts`` does not begin at 0, descends or passes
    ``n``; then nothing is taken anywhere.  No host read.

    ``mode=1``: the ordered rule (zk_front.h front_walk_ordered), in front of
    ``serve_sessions_mixed(ordered=True)``: writes do not end the run.  It is
    the longest prefix of whole frames, within ``quota``, up to a bad length,
    in which no CREATE / DELETE / SET_DATA follows a GET_CHILDREN,
    GET_CHILDREN2, GET_ACL (``has_acl``: the tree keeps an ACL table; without
    one GET_ACL is of the serve's class) or SET_WATCHES frame, and which a
    CLOSE_SESSION ends after itself.  ``nwr`` (int32 [S], required): the
    write frames taken.  ``mode=0`` launches what the call without the
    keywords does and leaves ``nwr`` alone.

    ``mode=2`` / ``mode=3``: modes 0 / 1 in front of a serve that takes
    SET_ACL (zk_front.h front_walk_setacl / front_walk_ordered_setacl): a
    SET_ACL frame is taken only as the first frame of a run and ends the run
    behind itself; ``nwr`` does not count it."""
    if mode == 0:
        lib().front_cut(raw, int(n), raw_starts, int(quota), int(max_packet),
                        take, nfr, flag, fault)
    else:
        lib().front_cut(raw, int(n), raw_starts, int(quota), int(max_packet),
                        take, nfr, flag, fault, int(mode), bool(has_acl), nwr)


def front_gather(streams, p_stream, p_src, p_off, P, dst, over):
    """Pack ``P`` pieces into ``dst`` (csrc/kernels/front.hip
    front_gather_k), on the current stream: piece i is ``p_off[i + 1] -
    p_off[i]`` bytes at ``p_src[i]`` of ``streams[p_stream[i]]`` (1 to 4
    uint8 tensors, one of no elements is absent; ``p_stream`` None: all of
    stream 0) and goes to ``dst[p_off[i]:p_off[i + 1]]``; ``p_off`` (int64
    [P + 1]) is the exclusive scan of the lengths with the total behind.  A
    piece that does not lie inside its stream is not copied.  ``over``
    (int64 [1]): 1 when the total is past ``dst.numel()``; then nothing is
    written.  No host read."""
    lib().front_gather(list(streams), p_stream, p_src, p_off, int(P), dst,
                       over)


def front_tx_pieces(rep_off, wslots, resume_off, notif_off, close_off, err,
                    caps, owner, p_stream, p_src, p_len, stats, rep_end=None):
    """The four pieces of every connection's bytes for its socket
    (csrc/kernels/front.hip; the rule: zk_front.h front_piece), on the
    current stream, in sending order: its replies ``rep_off[s]:rep_off[s +
    1]`` of stream 0, then watcher slot ``wslots[s]``'s slices of the
    catch-up, write-fired and close-fired notification streams (``*_off``:
    int64 [65]).  A slot's slices go to the lowest-numbered segment naming
    it; a second one gets none and is counted in ``stats[0]`` (int64 [8]).
    A ``wslots`` value outside 0..63 gets replies only, an absent table
    (None) or a batch whose ``err`` (int32 [1] or None) is not 0 gives
    empty pieces, and so does a slice outside ``caps`` (the four streams'
    bytes).  ``owner``: int64 [64] workspace.  Piece 4 s + k -> ``p_stream``
    (int32), ``p_src``, ``p_len`` (int64), each [4 S].  ``rep_end`` (int64
    [S] or None): connection s's replies end at ``rep_end[s]`` instead of
    ``rep_off[s + 1]`` (:func:`order_clip_ranges`).  No host read."""
    lib().front_tx_pieces(rep_off, wslots, resume_off, notif_off, close_off,
                          err, [int(c) for c in caps], owner, p_stream, p_src,
                          p_len, stats, rep_end)


def available():
    return os.path.exists(LIB_PATH) and os.path.exists(HIP_LIB_PATH)
