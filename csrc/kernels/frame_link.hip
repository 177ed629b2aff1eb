// K1's link pass: fs_link (the check of every tile's entry against the exit
// before it, the repair of broken links, the row bases) and its launch.  The
// design note: zk_frame_scan.h.
#include "zk_frame_scan.h"

namespace zk {

// Membership of crel in the sorted survivor list L[0..m0) (merge-walk: the
// walk only moves forward, so the 64-entry window lv only moves forward).
// Returns the list index or -1.
template <typename LoadL>
ZK_DEV int32_t fc_member(uint32_t crel, int32_t m0, int32_t& lb, uint32_t& lv,
                         int lane, LoadL loadL) {
  while (lb + 64 < m0 &&
         crel > (uint32_t)__builtin_amdgcn_readlane((int)lv, 63)) {
    lb += 64;
    lv = lb + lane < m0 ? loadL(lb + lane) : 0xFFFFFFFFu;
  }
  const uint64_t hit = __ballot(lv == crel);
  return hit ? lb + (int32_t)__builtin_ctzll(hit) : -1;
}

// What fs_link's steps need from the kernel (as fs_tile's FtCtx).
struct FlCtx {
  const uint8_t* buf;
  int64_t n, ntiles, maxp, cap;
  const int64_t* sx;
  const uint16_t* list;
  const int32_t* rcount;
  uint16_t* pre;
  int64_t *rec_entry, *rec_exit, *rec_meta;
  int64_t *base, *bsum;
  int64_t *result, *lastk;
  uint64_t* stats;
  int32_t* blist;
  const uint64_t* lbw;
  const int64_t* cx;
  int32_t* fblk;
  uint8_t* win;                   // LDS: a walk window per wave
  int64_t* red;                   // LDS: the block reductions' scratch
};

// fs_tile's join walk of tile k from global memory (a repair from the exact
// entry E), through a WIN-byte LDS window (4 KiB per wave: a tile in one
// staging).
template <int WIN = FC_WIN>
ZK_DEV FcWalk fc_walk(const FlCtx& C, int64_t k, int64_t E, uint8_t* win,
                      int lane) {
  const uint8_t* __restrict__ buf = C.buf;
  const int64_t n = C.n, maxp = C.maxp, ts = k * FT_S;
  const uint16_t* L = C.list + k * FT_LMAX;
  uint16_t* pre = C.pre + k * FT_LMAX;
  const int32_t m0 = __builtin_amdgcn_readfirstlane(C.rcount[k]);
  const int64_t send = C.sx[k];
  FcWalk r{E, 0, 0, -1, false, false};
  const int64_t tend = ts + FT_S;
  int64_t c = E;
  int64_t wb = -(int64_t)WIN;
  int32_t lb = 0;
  uint32_t lv = lane < m0 ? (uint32_t)L[lane] : 0xFFFFFFFFu;
  int32_t np = 0;
  for (;;) {
    if (c >= tend) { r.exit = c; break; }
    if (c >= n) { r.exit = n; break; }
    const uint32_t crel = (uint32_t)(c - ts);
    if (m0 > 0) {
      const int32_t j = fc_member(crel, m0, lb, lv, lane,
                                  [&](int i) { return (uint32_t)L[i]; });
      if (j >= 0) { r.js = j; break; }
    }
    if (c + 4 > n) { r.exit = c; r.term = true; break; }
    if (c < wb || c + 8 > wb + WIN) {
      wb = c & ~(int64_t)15;
      fc_stage<WIN>(buf, n, wb, win, lane);
    }
    const int32_t len =
        __builtin_amdgcn_readfirstlane(lds_be32(win, (int32_t)(c - wb)));
    if (len < 0 || (int64_t)len > maxp) {
      r.exit = c; r.term = true; r.bad = true; break;
    }
    const int64_t nx = c + 4 + len;
    if (nx > n) { r.exit = c; r.term = true; break; }
    if (lane == 0) pre[np] = (uint16_t)crel;
    ++np;
    c = nx;
  }
  r.np = np;
  r.cnt = np;
  if (r.js >= 0) {
    r.cnt = np + (m0 - r.js);
    fc_join_end(r, send, n);
  }
  return r;
}

// fs_link's grid: FL_BLOCKS workgroups check the links (fl_check), then
// each takes a ticket; the LAST block to arrive reads the check's minima
// and does the rest alone.  No block ever waits for another, so nothing
// depends on the grid being co-resident: a spin barrier here (rounds 2-4)
// waited for room beside the other connection's kernels (34 us in the
// overlapped GET step against 12 us alone, one 175 ms step on the watch
// stream).  The usual scan — no broken link before the first terminal —
// is the bases scan.  A repair: a handful of broken links are chased in
// parallel waves (fl_chase); more (every tile without a speculated entry,
// a run of garbage entries) go to the tail, which chases from the leftmost
// broken link with the exact entry — one wave looks a run of tiles up in
// fs_tile's candidate exits 64 at a time, walking only the tiles whose
// exact entry is not a candidate — until every live link holds.
// (A block re-walking the broken links its own check found before its
// ticket lost: the phantom-chain scan 0.27 -> 0.69 ms,
// profiles/r5_fs_link_ab.md.)
// Grid words (LW_GRID, uint64): [0] the ticket, [1] unused, [FL_NB] the
// check's count of broken links (fs_rows clears it for the next scan).
// At most this many broken links: chased from the check's list (fl_chase; a
// reply stream usually has a handful of broken links or none); more go to
// the tail's exact chases.
constexpr unsigned long long FL_SMALL = 1024;

// Is a repair walk of tile k (new exit x) written?  Always when the link
// before k holds (its entry E is then exact, or at least as good as the
// records get).  When that link is itself broken, E is suspect: a garbage
// exit of tile k-1 (say a frame-length read from an xid, megabytes ahead)
// walked on would break the link after k where it holds, that link's walk
// would break the next, and a wave of garbage would cross the stream one
// tile per round (the first storm reply stream: 1413 tiles re-walked over
// 71 rounds).  So a suspect walk that changes the exit is not written while
// link k+1 holds; link k stays broken for the last block's chases.  A walk
// from an E that tile k-1 has since replaced (another wave re-walked it at
// the same time) is stale and not written either.  (A refused walk has
// overwritten the tile's recorded frame starts all the same: its caller
// clears the entry.)
ZK_DEV bool fl_accept(const FlCtx& C, int64_t k, int64_t E, int64_t x) {
  if (ld_agent(&C.rec_exit[k - 1]) != E) return false;
  if (k < 2) return true;
  const bool suspect = ld_agent(&C.rec_entry[k - 1]) != ld_agent(&C.rec_exit[k - 2]);
  if (!suspect) return true;
  const int64_t ox = ld_agent(&C.rec_exit[k]);
  if (x == ox || k + 1 >= C.ntiles) return true;
  return ld_agent(&C.rec_entry[k + 1]) != ox;
}

// Tile k re-walked from entry E by one wave, its record written if the walk
// is accepted.
ZK_DEV void fl_rewalk(const FlCtx& C, int64_t k, int64_t E, uint8_t* mywin,
                      int lane) {
  const FcWalk fw = fc_walk(C, k, E, mywin, lane);
  if (lane != 0) return;
  if (fl_accept(C, k, E, fw.exit)) {
    st_agent(&C.rec_entry[k], E);
    st_agent(&C.rec_exit[k], fw.exit);
    st_agent(&C.rec_meta[k], fc_meta(fw));
  } else {
    // the walk overwrote the tile's frame starts (pre) while its record
    // keeps the old entry: no entry, so the link stays broken and the tile
    // is walked again (its exit, which the refusal protects, is kept)
    st_agent(&C.rec_entry[k], -1);
  }
}

// A repair round of the last block: the broken links blist[0, nloc), one
// wave a link.  Returns the tiles this wave re-walked.
ZK_DEV uint32_t fl_local_round(const FlCtx& C, int nloc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint8_t* mywin = C.win + (size_t)wv * (FC_WIN + 16);
  uint32_t walked = 0;
  for (int j = wv; j < nloc; j += FL_T / 64) {
    const int64_t k = C.blist[j];
    const int64_t E = wave_uniform(ld_agent(&C.rec_exit[k - 1]));
    if (E < k * FT_S ||
        __builtin_amdgcn_readfirstlane(m_term(ld_agent(&C.rec_meta[k - 1]))))
      continue;                               // no usable entry yet
    fl_rewalk(C, k, E, mywin, lane);
    ++walked;
  }
  return walked;
}

// ---- the big repair ---------------------------------------------------------
// A scan with hundreds of tiles without a speculated entry (adversarial
// streams: every payload word a plausible length, tests that withhold
// every entry) needs the grid's parallelism round after round, which no
// single block has: there the grid keeps the barrier rounds of rounds 2-4.
// The decision comes from fs_tile's count of this scan, known before
// fs_link starts, so every block takes the same path and no ordinary scan
// ever waits in a barrier.  Barrier words (LW_BIG, uint64): [0] arrivals,
// [1] generation, [2] abort, [4 + 2r] the links round r listed.
constexpr uint64_t FL_BAR_TICKS = 50000000;   // 0.5 s: barrier abandoned

// Grid barrier over fs_link's workgroups (16: they find CUs beside
// anything else that runs, and nothing they wait for needs a CU they hold).
// Every wait is bounded: past FL_BAR_TICKS the grid is told to abort and
// block 0 falls back to the serial repair.  Returns false on abort.
ZK_DEV bool fl_sync(unsigned long long* g) {
  __shared__ int s_ok;
  __syncthreads();
  if (threadIdx.x == 0) {
    int ok = 1;
    __threadfence();
    const unsigned long long gen =
        __hip_atomic_load(&g[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long a =
        __hip_atomic_fetch_add(&g[0], 1ull, __ATOMIC_ACQ_REL,
                               __HIP_MEMORY_SCOPE_AGENT) + 1;
    if (a == gridDim.x) {
      __hip_atomic_store(&g[0], 0ull, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&g[1], 1ull, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_AGENT);
    } else {
      const uint64_t t0 = wall_clock64();
      while (__hip_atomic_load(&g[1], __ATOMIC_ACQUIRE,
                               __HIP_MEMORY_SCOPE_AGENT) == gen) {
        if (__hip_atomic_load(&g[2], __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT)) {
          ok = 0;
          break;
        }
        if (wall_clock64() - t0 > FL_BAR_TICKS) {
          __hip_atomic_store(&g[2], 1ull, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(8);
      }
    }
    __threadfence();
    if (__hip_atomic_load(&g[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      ok = 0;
    s_ok = ok;
  }
  __syncthreads();
  return s_ok != 0;
}

// One grid repair round (every thread of every block calls it).  Returns
// false when no link was broken (the fix-point is reached) or on abort.
ZK_DEV bool fl_round(const FlCtx& C, unsigned long long* g, int r) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t nblk = gridDim.x;
  const int64_t bid = blockIdx.x;
  const int64_t nth = nblk * FL_T;
  const int64_t gt = bid * FL_T + tid;
  // B. list the broken links (after a tile that is not a terminal).  Every
  // one, not only those before the first terminal: a terminal may be a
  // speculation's (a garbage entry that died) that this very round fixes,
  // and stopping the list there made a stream with many such tiles take a
  // round per terminal (26 ms a 0-1024 B reply stream at a 1 KiB window).
  // Past a real bad frame the walks are wasted, and the serial tail's
  // first terminal bounds what counts.
  int64_t nb = 0;
  const int64_t per = (C.ntiles - 1 + nth - 1) / nth;
  const int64_t k0 = 1 + gt * per, k1 = min(k0 + per, C.ntiles);
  auto broken = [&](int64_t k) {
    return ld_agent(&C.rec_entry[k]) != ld_agent(&C.rec_exit[k - 1]) &&
           !m_term(ld_agent(&C.rec_meta[k - 1]));
  };
  for (int64_t k = k0; k < k1; ++k) nb += broken(k);
  int64_t tot;
  const int64_t o = block_excl_scan(nb, C.red, &tot);
  __shared__ unsigned long long s_base;
  if (tid == 0)
    s_base = tot ? atomicAdd(&g[4 + 2 * r], (unsigned long long)tot) : 0;
  __syncthreads();
  int64_t w = (int64_t)s_base + o;
  for (int64_t k = k0; k < k1; ++k)
    if (broken(k)) C.blist[w++] = (int32_t)k;
  if (!fl_sync(g)) return false;
  const int64_t nbr = (int64_t)__hip_atomic_load(
      &g[4 + 2 * r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (nbr == 0) return false;
  // C. every listed link re-walked by one wave, from the exit before it
  uint8_t* mywin = C.win + (size_t)wv * (FC_WIN + 16);
  const int64_t nwv = nblk * (FL_T / 64);
  uint32_t walked = 0;
  for (int64_t j = bid * (FL_T / 64) + wv; j < nbr; j += nwv) {
    const int64_t k = C.blist[j];
    const int64_t E = ld_agent(&C.rec_exit[k - 1]);
    if (E < k * FT_S) continue;               // no exact entry yet
    fl_rewalk(C, k, E, mywin, lane);
    ++walked;
  }
  if (lane == 0 && walked) fc_stat(C.stats, 2, walked);
  if (bid == 0 && tid == 0) fc_stat(C.stats, 3, 1);
  return fl_sync(g);
}

// The full check (fs_link, when fs_tile counted a bad link): every link and
// terminal, one wave per count block of FK_T tiles over the grid, and the
// frame counts scanned per block: base[k] = count before tile k within its
// block, bsum[b] = the block's total.  The leftmost broken link and terminal
// go to mins[0..1] as (ntiles - k) maxima, the broken links to blist (their
// count in *nbroken).  Cross-block data: agent-scope stores (the blocks may
// sit on different XCDs, each with its own L2).
ZK_DEV void fl_check(const FlCtx& C, uint64_t* mins,
                     unsigned long long* nbroken) {
  const int lane = threadIdx.x & 63;
  const int64_t INF = INT64_MAX;
  const int64_t nw = (int64_t)gridDim.x * (FL_T / 64);
  const int64_t nbl = (C.ntiles + FK_T - 1) / FK_T;
  int64_t fb = INF, fterm = INF;
  for (int64_t b = (int64_t)blockIdx.x * (FL_T / 64) + (threadIdx.x >> 6);
       b < nbl; b += nw) {
    const int64_t k = b * FK_T + lane;
    int64_t cnt = 0;
    bool brk = false;
    if (k < C.ntiles) {
      // written by fs_tile (an earlier launch): plain loads, issued together
      const int64_t mk = C.rec_meta[k];
      const bool nxt = k + 1 < C.ntiles;
      const int64_t e = nxt ? C.rec_entry[k + 1] : 0;
      const int64_t x = C.rec_exit[k];
      cnt = m_cnt(mk);
      if (m_term(mk)) {
        fterm = min(fterm, k);
      } else if (nxt && (e < 0 || e != x)) {
        brk = true;
        fb = min(fb, k + 1);
      }
    }
    const uint64_t bm = __ballot(brk);
    if (bm) {
      unsigned long long b0 = 0;
      if (lane == 0) b0 = atomicAdd(nbroken, (unsigned long long)__popcll(bm));
      b0 = __shfl(b0, 0, 64);
      if (brk) {
        const uint64_t below = lane ? (bm & ((~0ull) >> (64 - lane))) : 0ull;
        __hip_atomic_store(&C.blist[b0 + __popcll(below)], (int32_t)(k + 1),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    const int64_t inc = wave_incl_scan(cnt);
    if (k < C.ntiles) st_agent(&C.base[k], inc - cnt);
    if (lane == 63) st_agent(&C.bsum[b], inc);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    fb = min(fb, (int64_t)__shfl_xor(fb, d, 64));
    fterm = min(fterm, (int64_t)__shfl_xor(fterm, d, 64));
  }
  if (lane == 0) {
    if (fb != INF) atomicMax((unsigned long long*)&mins[0],
                             (unsigned long long)(C.ntiles - fb));
    if (fterm != INF) atomicMax((unsigned long long*)&mins[1],
                                (unsigned long long)(C.ntiles - fterm));
  }
}

// Row bases once every link up to the first terminal ft (INF: none) holds:
// bsum[b] (block b's count total, the check's or re-counted) becomes block
// b's exclusive offset; base[k] stays the in-block one; result[0..3] and
// the last tile; and the frame-block index (ZkFrameTiles.fblk: a scatter of
// frames / 256 words, each block's thread writing those of its own rows).
// fs_link's last block alone.
ZK_DEV void fl_bases(const FlCtx& C, int64_t ft) {
  const int tid = threadIdx.x;
  const int64_t INF = INT64_MAX;
  const int64_t last = ft == INF ? C.ntiles - 1 : ft;
  const int64_t nbl = last / FK_T + 1;
  const int64_t per = (nbl + FL_T - 1) / FL_T;
  const int64_t b0 = (int64_t)tid * per;
  const int64_t b1 = min(b0 + per, nbl);
  int64_t sum = 0;
  for (int64_t b = b0; b < b1; ++b) sum += ld_agent(&C.bsum[b]);
  int64_t tot;
  int64_t run = block_excl_scan(sum, C.red, &tot);
  const int64_t blast = last / FK_T;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t v = ld_agent(&C.bsum[b]);
    C.bsum[b] = run;
    int64_t live = v;                       // the block's rows
    if (b == blast) {
      // frames up to `last` (tiles after it in its block are dead)
      const int64_t ml = ld_agent(&C.rec_meta[last]);
      const int64_t total = run + ld_agent(&C.base[last]) + m_cnt(ml);
      live = total - run;
      *C.lastk = last;
      C.result[0] = total;
      C.result[3] = total > C.cap ? 1 : 0;
      if (ft == INF) {
        C.result[1] = C.n;
        C.result[2] = 0;
      } else {
        C.result[1] = ld_agent(&C.rec_exit[ft]);
        C.result[2] = m_bad(ml) ? 1 : 0;
      }
    }
    for (int64_t j = (run + FR_T - 1) / FR_T; j * FR_T < run + live; ++j)
      C.fblk[j] = (int32_t)b;
    run += v;
  }
}

// The small repair (a handful of broken links, the usual kind): CHASES.
// The check listed the broken links.  A chase starts at one with the exact
// entry (the exit before it) and runs forward while the link after the
// tile it settled is still broken.  Most tiles of a run need no walk:
// their exact entry is one of the candidate entries fs_tile walked, whose
// exit and frame count `cx` already holds (fs_tile's entry -> exit map),
// so the chase only looks it up — a wave loads the candidate words and
// exits of 64 tiles at once and resolves them with a 6-step parallel
// prefix over the tiles' slot maps.  A tile whose entry is not a candidate
// (a frame longer than the window) is walked; tiles a long frame covers
// whole are filled in one step.  Looked-up tiles are marked stale: fs_rows
// walks their frame starts, in parallel with every other tile.  (Round 3
// first re-walked every tile of a run one after the other: on the storm's
// phantom-chain replies, 650 tiles in 18 ms; then looked them up one tile
// at a time, ~0.3 us each.)
// Chases of different runs run in parallel (one wave each) in rounds: a
// round's chases, then a check of every run's first and last link (another
// run may have moved an exit), the broken ones (deduplicated in an LDS
// hash set) chased next round.  Only the count blocks holding a re-written
// tile are re-counted.  When the lists outgrow LDS or the rounds run out,
// fs_link's tail (exact chases from the leftmost broken link) finishes from
// the records as they stand.
constexpr int FL_WL = 1024;                // chases per round
constexpr int FL_HS = 2048;                // their dedup hash set
constexpr int FL_WR = 48;                  // rounds before the tail
constexpr int FL_DB = 8192;                // count blocks tracked (2M tiles)
static_assert(FL_SMALL <= FL_WL, "the check's list fits the first round");

struct FlChase {
  uint32_t* dirty;                // count blocks holding re-written tiles
  int* overflow;
  uint64_t* stats;
  int64_t* clk;                   // ZKMI_FS_DBG: the exact chase's span
};

ZK_DEV void fl_dirty(FlChase& ch, int64_t t) {
  const int64_t b = t / FK_T;
  // (past FL_DB count blocks only the tail chases, which re-counts all)
  if (b < FL_DB) atomicOr(&ch.dirty[b >> 5], 1u << (b & 31));
}

ZK_DEV int live_count(const int64_t* c5) {
  int live = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) live += c5[j] != FC_DEAD;
  return live;
}


ZK_DEV uint64_t readlane64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi =
      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// One chase (one wave) from broken link k0.  Returns the last tile it
// wrote (-1: none), `term` when that tile ends the chain.
// `exact`: k0 is the round's leftmost broken link, so its entry (the exit
// before it) is exact and so is everything the chase derives.  It stops at
// a link that holds only where the tile after is unambiguous (one live
// candidate): a run of tiles where two chains both survive (a phantom
// chain) can hold links that are consistent and wrong, and only a chase
// from an exact entry can tell — it goes through the whole run.
// Otherwise (another broken link of the round, entry not known exact) the
// chase writes nothing that would break a link that holds (a phantom's
// exit must not run over a true segment: a garbage exit walked on would
// break the link after it, and a wave of garbage would cross the stream one
// tile per round); it stops there and the link waits for a later round.
ZK_DEV int64_t fl_chase_run(const FlCtx& C, uint8_t* mywin, FlChase& ch,
                            int64_t k0, bool exact, bool& term,
                            uint32_t& walked, uint32_t walk_budget = 0) {
  // (its records and maps by name, read once)
  const int64_t ntiles = C.ntiles;
  int64_t* rec_entry = C.rec_entry;
  int64_t* rec_exit = C.rec_exit;
  int64_t* rec_meta = C.rec_meta;
  const uint64_t* lbw = C.lbw;
  const int64_t* cx = C.cx;
  const int lane = threadIdx.x & 63;
  term = false;
  // everything that steers the chase is wave-uniform; saying so keeps its
  // control flow scalar (else the compiler runs the batch loop below as
  // divergent code under exec masks: ~850 cycles a tile)
  k0 = wave_uniform(k0);
  exact = __builtin_amdgcn_readfirstlane((int)exact) != 0;
  int64_t k = k0;
  int64_t E = wave_uniform(ld_agent(&rec_exit[k - 1]));
  if (E < k * FT_S ||
      __builtin_amdgcn_readfirstlane(m_term(ld_agent(&rec_meta[k - 1]))))
    return -1;
  if (!exact && wave_uniform(ld_agent(&rec_entry[k])) == E) return -1;  // holds
  bool first = true;             // tile k0's own link is the broken one
  for (;;) {
    if (E >= (k + 1) * FT_S) {
      // a frame covers tiles k .. kx-1 whole: no frame starts there.  (Only
      // from an exact entry: a garbage exit megabytes ahead would wipe out
      // every tile it claims to cover.)
      if (!exact) return k - 1;
      const int64_t kend = min(E / FT_S, ntiles);
      const FcWalk cov{E, 0, 0, -1, false, false};
      for (int64_t c = k + lane; c < kend; c += 64) {
        st_agent(&rec_entry[c], E);
        st_agent(&rec_exit[c], E);
        st_agent(&rec_meta[c], fc_meta(cov));
        fl_dirty(ch, c);
      }
      if (kend >= ntiles) return kend - 1;
      k = kend;
      first = false;
      continue;
    }
    // ---- a batch of 64 tiles, lane i = tile k+i ------------------------
    // Each lane loads its tile's candidate word (written by the tile
    // before), the five candidate exits, its entry and exit and the next
    // tile's entry, and turns them into a transition table over its five
    // candidate slots: the slot of the next tile that each exit enters
    // (next lane's word), whether the link into this tile holds with that
    // slot's entry, whether taking it would break a holding link, whether
    // two candidates survive.  The serial walk over the batch is then a
    // few scalar instructions a tile.  (Round 3 first resolved each tile
    // from the raw words: ~150 dependent instructions, 0.6 us a tile.)
    const int64_t tl = k + lane;
    const int64_t ts_l = tl * FT_S;
    uint64_t wd = 0;
    int64_t en = INT64_MIN, ent = INT64_MIN, ox = INT64_MIN + 1;
    int64_t c5[5];               // candidate exits
    int32_t n5[5];               // and their frame counts
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      c5[j] = FC_DEAD;
      n5[j] = 0;
    }
    if (tl < ntiles) {
      wd = lb_load(&lbw[2 * (tl - 1)]);
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int64_t v = cx[5 * tl + j];
        c5[j] = cx_exit(v);
        n5[j] = cx_cnt(v);
      }
      ent = ld_agent(&rec_entry[tl]);
      ox = ld_agent(&rec_exit[tl]);
    }
    if (tl + 1 < ntiles) en = ld_agent(&rec_entry[tl + 1]);
    // the next tile's slots
    const uint32_t wn_lo = (uint32_t)__shfl_down((int)(uint32_t)wd, 1, 64);
    const uint32_t wn_hi =
        (uint32_t)__shfl_down((int)(uint32_t)(wd >> 32), 1, 64);
    const uint64_t wn = ((uint64_t)wn_hi << 32) | wn_lo;
    const int64_t tend_l = ts_l + FT_S;
    const bool next_holds = tl + 1 < ntiles && en == ox;
    // lane i's map M over the state of its tile — the entry slot 0..4, or
    // 5 stopped (an earlier tile ended the run), 6 walk (the entry is the
    // exit before, not among the candidates), 7 leave (the entry lies
    // past the tile or the batch) — to the state of the tile after it.
    // Tile i stops the run (maps to 5) when its link already holds with
    // that entry (an exact chase goes on through ambiguous tiles), when a
    // non-exact chase would break a holding link, or when the exit is not
    // known (the tile is walked).
    const bool amb = live_count(c5) >= 2;
    const bool head = first && lane == 0;   // k0: its link is the broken one
    uint32_t M = (5u << 15) | (5u << 18) | (5u << 21);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const uint32_t oj = (uint32_t)((wd >> (12 * j)) & 0xFFF);  // off + 1
      const int64_t xj = c5[j];
      uint32_t nx = 5;                      // (no looked-up exit: stops)
      if (tl < ntiles && oj != 0 && xj >= tend_l) {
        if (xj >= tend_l + FT_S || lane == 63 || tl + 1 >= ntiles) {
          nx = 7;
        } else {
          const uint32_t want = (uint32_t)(xj - tend_l) + 1;
          nx = 6;
#pragma unroll
          for (int q = 4; q >= 0; --q)
            if ((uint32_t)((wn >> (12 * q)) & 0xFFF) == want) nx = q;
        }
        const bool holds = ent == ts_l + (int64_t)oj - 1;
        if (!head && holds && !(exact && amb)) nx = 5;
        if (!exact && xj != ox && next_holds) nx = 5;
      }
      M |= nx << (3 * j);
    }
    // the state of the batch's first tile
    uint32_t j0 = 6;
    {
      const uint64_t w0 = readlane64(wd, 0);
      const uint32_t want = (uint32_t)(E - k * FT_S) + 1;
#pragma unroll
      for (int q = 4; q >= 0; --q)
        if ((uint32_t)((w0 >> (12 * q)) & 0xFFF) == want) j0 = q;
    }
    // prefix composition over the lanes (Hillis-Steele, 6 steps): T_i =
    // M_i o ... o M_0; the state of tile i is T_{i-1}(j0)
    uint32_t T = M;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t U = (uint32_t)__shfl_up((int)T, d, 64);
      if (lane >= d) {
        uint32_t C = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          C |= ((T >> (3 * ((U >> (3 * q)) & 7))) & 7) << (3 * q);
        T = C;
      }
    }
    const uint32_t Tp = (uint32_t)__shfl_up((int)T, 1, 64);
    const uint32_t st = lane == 0 ? j0 : (Tp >> (3 * j0)) & 7;
    // looked up: a tile whose state is an entry slot and whose map does not
    // stop there
    const bool mine = tl < ntiles && st < 5 && ((M >> (3 * st)) & 7) != 5;
    const uint64_t looked = __ballot(mine);
    // the run of looked-up tiles is a prefix of the batch
    const int f = looked == ~0ull ? 64 : (int)__builtin_ctzll(~looked);
    if (f > 0) {
      if (lane == 0) fc_stat(ch.stats, 0, (uint32_t)f);
      if (lane < f) {
        // exact entry, exit and frame count; the frame starts themselves
        // are walked by fs_rows (a stale tile)
        const uint32_t oj = (uint32_t)((wd >> (12 * st)) & 0xFFF);
        const int64_t xj = st == 0 ? c5[0] : st == 1 ? c5[1]
                           : st == 2 ? c5[2] : st == 3 ? c5[3] : c5[4];
        const int32_t nj = st == 0 ? n5[0] : st == 1 ? n5[1]
                           : st == 2 ? n5[2] : st == 3 ? n5[3] : n5[4];
        st_agent(&rec_entry[tl], ts_l + (int64_t)oj - 1);
        st_agent(&rec_exit[tl], xj);
        st_agent(&rec_meta[tl], M_STALE | nj);
        fl_dirty(ch, tl);
      }
      first = false;
    }
    if (k + f >= ntiles) return ntiles - 1;
    // what ends the run at tile k+f: its state
    const uint32_t sf = (uint32_t)__builtin_amdgcn_readlane((int)st, f & 63);
    if (f < 64 && sf < 5) {
      // its map stops there: the link holds, a refusal, or no known exit
      const uint32_t oj = (uint32_t)((readlane64(wd, f) >> (12 * sf)) & 0xFFF);
      const int64_t xs = (int64_t)readlane64(
          (uint64_t)(sf == 0 ? c5[0] : sf == 1 ? c5[1] : sf == 2 ? c5[2]
                     : sf == 3 ? c5[3] : c5[4]), f);
      if (xs >= (k + f + 1) * FT_S) return k + f - 1;   // link / refusal
      E = (k + f) * FT_S + (int64_t)oj - 1;              // walked below
    } else {
      // 6 / 7 (or the batch done): the entry is the exit before it
      const int l = f - 1;
      const uint32_t sl =
          (uint32_t)__builtin_amdgcn_readlane((int)st, l < 0 ? 0 : l);
      if (l >= 0)
        E = (int64_t)readlane64(
            (uint64_t)(sl == 0 ? c5[0] : sl == 1 ? c5[1] : sl == 2 ? c5[2]
                       : sl == 3 ? c5[3] : c5[4]), l);
    }
    k += f;
    if (f == 64 || sf == 7) continue;          // next batch / covered

    // stop == 2: tile k (entry E) is walked
    {
      const int64_t t = k;
      if (t >= ntiles) return t - 1;
      if (E >= (t + 1) * FT_S) continue;          // covered: to the top
      if (!first && wave_uniform(ld_agent(&rec_entry[t])) == E && !exact)
        return t - 1;
      const int64_t oldx = wave_uniform(ld_agent(&rec_exit[t]));
      const bool nh = t + 1 < ntiles &&
                      wave_uniform(ld_agent(&rec_entry[t + 1])) == oldx;
      // (a budgeted chase leaves the walking to the caller's rounds)
      if (walk_budget != 0 && walked >= walk_budget) return t - 1;
      const FcWalk fw = fc_walk(C, t, E, mywin, lane);
      ++walked;
      if (!exact && wave_uniform(fw.exit) != oldx && nh) {
        // refused, but the walk overwrote the tile's frame starts (pre)
        // while its record keeps the old entry: no entry, so its link stays
        // broken and the tile is walked again
        if (lane == 0) st_agent(&rec_entry[t], -1);
        return t - 1;
      }
      if (lane == 0) {
        st_agent(&rec_entry[t], E);
        st_agent(&rec_exit[t], fw.exit);
        st_agent(&rec_meta[t], fc_meta(fw));
        fl_dirty(ch, t);
      }
      first = false;
      if (__builtin_amdgcn_readfirstlane(fw.term)) { term = true; return t; }
      if (t + 1 >= ntiles) return t;
      // an exact chase stops where the next link holds and the tile after
      // has one live candidate; the next batch checks that
      E = wave_uniform(fw.exit);
      k = t + 1;
    }
  }
}

// fs_link's last block: chase rounds to a fix-point of the links.  Returns
// false when it gave up (the tail takes over).
ZK_DEV bool fl_chase(const FlCtx& C, int nb0, FlChase& ch) {
  __shared__ int32_t wl[2][FL_WL];
  __shared__ int32_t wk[FL_WL];              // run ends (+ 1; 0: none)
  __shared__ uint32_t hs[FL_HS];
  __shared__ int s_n;
  __shared__ int s_cur;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // the check's list to LDS
  for (int i = tid; i < nb0; i += FL_T)
    wl[0][i] = __hip_atomic_load(&C.blist[i], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) s_cur = nb0;
  uint8_t* mywin = C.win + (size_t)wv * (FC_WIN + 16);
  int cur = 0, rounds = 0;
  uint32_t walked = 0;
  __syncthreads();
  int ncur = s_cur;
  while (ncur > 0) {
    if (rounds == FL_WR) break;
    ++rounds;
    const int nxt = cur ^ 1;
    for (int i = tid; i < FL_HS; i += FL_T) hs[i] = 0;
    if (tid == 0) s_n = 0;
    __syncthreads();
    // one lane lists link k for the next round (once)
    auto push = [&](int64_t k) {
      const uint32_t key = (uint32_t)k + 1;
      uint32_t h = (key * 2654435761u) >> (32 - 11);
      for (;;) {
        const uint32_t old = atomicCAS(&hs[h], 0u, key);
        if (old == 0) break;
        if (old == key) return;
        h = (h + 1) & (FL_HS - 1);
      }
      const int i = atomicAdd(&s_n, 1);
      if (i < FL_WL) wl[nxt][i] = (int32_t)k;
      else *ch.overflow = 1;
    };
    // the round's leftmost broken link: its entry is exact
    int32_t lo = INT32_MAX;
    for (int j = lane; j < ncur; j += 64) lo = min(lo, wl[cur][j]);
    for (int d = 32; d >= 1; d >>= 1) lo = min(lo, __shfl_xor(lo, d, 64));
    for (int j = wv; j < ncur; j += FL_T / 64) {
      bool term;
      const bool ex = wl[cur][j] == lo;
      if (ex && ch.clk && lane == 0) ch.clk[6] = wall_clock64();
      const int64_t kend = fl_chase_run(C, mywin, ch, wl[cur][j],
                                        wl[cur][j] == lo, term, walked);
      if (ex && ch.clk && lane == 0) ch.clk[7] = wall_clock64();
      if (lane == 0)
        wk[j] = kend < 0 ? 0 : (int32_t)(kend + 1) | (term ? (1 << 30) : 0);
    }
    __syncthreads();
    // every run's first and last link, as the records stand now
    for (int j = tid; j < ncur; j += FL_T) {
      const int64_t k0 = wl[cur][j];
      if (ld_agent(&C.rec_entry[k0]) != ld_agent(&C.rec_exit[k0 - 1]) &&
          !m_term(ld_agent(&C.rec_meta[k0 - 1])))
        push(k0);
      const int32_t e = wk[j];
      if (e == 0 || (e & (1 << 30))) continue;
      const int64_t kend = (e & ((1 << 30) - 1)) - 1;
      if (kend + 1 < C.ntiles &&
          ld_agent(&C.rec_entry[kend + 1]) != ld_agent(&C.rec_exit[kend]))
        push(kend + 1);
    }
    __syncthreads();
    if (tid == 0) s_cur = *ch.overflow ? -1 : s_n;
    __syncthreads();
    ncur = s_cur;
    cur = nxt;
    __syncthreads();
    if (ncur < 0) break;
  }
  if (lane == 0 && walked) fc_stat(C.stats, 2, walked);
  if (tid == 0 && rounds) fc_stat(C.stats, 3, rounds);
  return ncur == 0 && !*ch.overflow;
}

// After the chases and the check of every link (the last block): re-count
// the count blocks holding a re-written tile, one wave per block, a tile per
// lane.
ZK_DEV void fl_chase_recount(const FlCtx& C, FlChase& ch) {
  static_assert(FK_T == 64, "a count block is a wave");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nbl = (C.ntiles + FK_T - 1) / FK_T;
  for (int64_t b = wv; b < nbl; b += FL_T / 64) {
    if (!((ch.dirty[b >> 5] >> (b & 31)) & 1u)) continue;
    const int64_t k = b * FK_T + lane;
    const int64_t c = k < C.ntiles ? m_cnt(ld_agent(&C.rec_meta[k])) : 0;
    const int64_t inc = wave_incl_scan(c);
    if (k < C.ntiles) st_agent(&C.base[k], inc - c);
    if (lane == 63) st_agent(&C.bsum[b], inc);
  }
  __syncthreads();
}

// Every live link holds up to the first terminal ft (INF: none): the
// exclusive scan of the counts of tiles 0..ft as absolute row bases (bsum
// zero: fs_rows adds no block offset), tiles after ft dead; result[0..3]
// the last tile and the frame-block index (as fl_bases).  The last block
// alone, after a repair.
ZK_DEV void fl_count_scan(const FlCtx& C, int64_t ft) {
  const int tid = threadIdx.x;
  const int64_t INF = INT64_MAX;
  const int64_t last = ft == INF ? C.ntiles - 1 : ft;
  const int64_t per = (last + 1 + FL_T - 1) / FL_T;
  const int64_t k0 = (int64_t)tid * per;
  const int64_t k1 = min(k0 + per, last + 1);
  int64_t sum = 0;
  for (int64_t kb = k0; kb < k1; kb += FL_U) {
    int64_t v[FL_U];
#pragma unroll
    for (int u = 0; u < FL_U; ++u)
      v[u] = kb + u < k1 ? ld_agent(&C.rec_meta[kb + u]) : 0;
#pragma unroll
    for (int u = 0; u < FL_U; ++u) sum += m_cnt(v[u]);
  }
  int64_t tot;
  int64_t run = block_excl_scan(sum, C.red, &tot);
  for (int64_t kb = k0; kb < k1; kb += FL_U) {
    int64_t v[FL_U];
#pragma unroll
    for (int u = 0; u < FL_U; ++u)
      v[u] = kb + u < k1 ? ld_agent(&C.rec_meta[kb + u]) : 0;
#pragma unroll
    for (int u = 0; u < FL_U; ++u) {
      if (kb + u < k1) C.base[kb + u] = run;
      const int64_t end = run + m_cnt(v[u]);
      for (int64_t j = (run + FR_T - 1) / FR_T; j * FR_T < end; ++j)
        C.fblk[j] = (int32_t)((kb + u) / FK_T);
      run = end;
    }
  }
  for (int64_t k = last + 1 + tid; k < C.ntiles; k += FL_T) C.base[k] = -1;
  for (int64_t b = tid; b <= last / FK_T; b += FL_T) C.bsum[b] = 0;
  if (tid == 0) {
    *C.lastk = last;
    C.result[0] = tot;
    C.result[3] = tot > C.cap ? 1 : 0;
    if (ft == INF) {
      C.result[1] = C.n;
      C.result[2] = 0;
    } else {
      // (a stop before a tile that is no terminal — unreachable, see the
      // tail — leaves the carry at tile ft's exit)
      const int64_t mf = ld_agent(&C.rec_meta[ft]);
      C.result[1] = ld_agent(&C.rec_exit[ft]);
      C.result[2] = m_term(mf) && m_bad(mf) ? 1 : 0;
    }
  }
}

// The block's minima of the threads' leftmost broken link and terminal.
ZK_DEV void fl_block_min(int64_t* red, int64_t fb, int64_t fterm,
                         int64_t& fb_out, int64_t& ft_out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int d = 32; d >= 1; d >>= 1) {
    fb = min(fb, (int64_t)__shfl_xor(fb, d, 64));
    fterm = min(fterm, (int64_t)__shfl_xor(fterm, d, 64));
  }
  if (lane == 0) { red[wv] = fb; red[FL_T / 64 + wv] = fterm; }
  __syncthreads();
  fb = INT64_MAX;
  fterm = INT64_MAX;
  for (int j = 0; j < FL_T / 64; ++j) {
    fb = min(fb, red[j]);
    fterm = min(fterm, red[FL_T / 64 + j]);
  }
  __syncthreads();
  fb_out = fb;
  ft_out = fterm;
}

// The leftmost terminal, and the leftmost broken link at or after `from`
// (INF: none), over the whole block.  Loads in batches of FL_U tiles a
// thread, all issued before any is used (one round trip a batch).
ZK_DEV void fl_links(const FlCtx& C, int64_t from, int64_t& fb_out,
                     int64_t& ft_out) {
  const int tid = threadIdx.x;
  const int64_t INF = INT64_MAX;
  int64_t fb = INF, fterm = INF;
  for (int64_t k0 = max(from - 1, (int64_t)0) + tid; k0 < C.ntiles;
       k0 += FL_U * FL_T) {
    int64_t mk[FL_U], e[FL_U], x[FL_U];
#pragma unroll
    for (int u = 0; u < FL_U; ++u) {
      const int64_t k = k0 + (int64_t)u * FL_T;
      const bool in = k < C.ntiles, nx = k + 1 < C.ntiles;
      mk[u] = in ? ld_agent(&C.rec_meta[k]) : 0;
      e[u] = nx ? ld_agent(&C.rec_entry[k + 1]) : 0;
      x[u] = in ? ld_agent(&C.rec_exit[k]) : 0;
    }
#pragma unroll
    for (int u = 0; u < FL_U; ++u) {
      const int64_t k = k0 + (int64_t)u * FL_T;
      if (k >= C.ntiles) break;
      if (m_term(mk[u])) {
        fterm = min(fterm, k);
      } else if (k + 1 < C.ntiles && k + 1 >= from) {
        if (e[u] < 0 || e[u] != x[u]) fb = min(fb, k + 1);
      }
    }
  }
  fl_block_min(C.red, fb, fterm, fb_out, ft_out);
}

// Every broken link (after a tile that is no terminal) into blist, in tile
// order, by the whole block; returns their count.  fb / ft: the leftmost
// broken link and terminal (INF: none).
ZK_DEV int64_t fl_list_broken(const FlCtx& C, int64_t& fb_out,
                              int64_t& ft_out) {
  const int tid = threadIdx.x;
  const int64_t INF = INT64_MAX;
  // a thread's run of tiles, its loads in batches of FL_U (all issued
  // before any is used) — this runs once per repair round
  const int64_t per = (C.ntiles + FL_T - 1) / FL_T;
  const int64_t k0 = (int64_t)tid * per, k1 = min(k0 + per, C.ntiles);
  int64_t cnt = 0, fb = INF, fterm = INF;
  for (int pass = 0; pass < 2; ++pass) {
    int64_t w = 0;
    if (pass == 1) {
      int64_t tot;
      w = block_excl_scan(cnt, C.red, &tot);
      C.red[2 * (FL_T / 64) + 1] = tot;       // (read after the loop)
      if (cnt == 0) break;
    }
    for (int64_t kb = k0; kb < k1; kb += FL_U) {
      int64_t mp[FL_U], mk[FL_U], e[FL_U], x[FL_U];
#pragma unroll
      for (int u = 0; u < FL_U; ++u) {
        const int64_t k = kb + u;
        const bool in = k < k1;
        mk[u] = in ? ld_agent(&C.rec_meta[k]) : 0;
        mp[u] = in && k >= 1 ? ld_agent(&C.rec_meta[k - 1]) : 0;
        e[u] = in ? ld_agent(&C.rec_entry[k]) : 0;
        x[u] = in && k >= 1 ? ld_agent(&C.rec_exit[k - 1]) : 0;
      }
#pragma unroll
      for (int u = 0; u < FL_U; ++u) {
        const int64_t k = kb + u;
        if (k >= k1) break;
        const bool brk = k >= 1 && !m_term(mp[u]) && e[u] != x[u];
        if (pass == 0) {
          if (brk) { ++cnt; fb = min(fb, k); }
          if (m_term(mk[u])) fterm = min(fterm, k);
        } else if (brk) {
          C.blist[w++] = (int32_t)k;
        }
      }
    }
  }
  __syncthreads();
  const int64_t total = C.red[2 * (FL_T / 64) + 1];
  __syncthreads();
  fl_block_min(C.red, fb, fterm, fb_out, ft_out);
  return total;
}

__global__ __launch_bounds__(FL_T) void fs_link(
    const uint8_t* __restrict__ buf, const int64_t* __restrict__ n_dev,
    int64_t n_cap, int64_t maxp, const int64_t* __restrict__ sx,
    const uint16_t* __restrict__ list, const int32_t* __restrict__ rcount,
    uint16_t* pre, int64_t* rec_entry, int64_t* rec_exit, int64_t* rec_meta,
    int64_t* __restrict__ base, int64_t cap, int64_t* __restrict__ result,
    uint64_t* stats, int32_t* __restrict__ blist,
    int64_t* __restrict__ bsum, uint64_t* mins,
    int64_t* __restrict__ lastk, unsigned long long* g,
    const uint64_t* lbw, const int64_t* __restrict__ cx,
    int64_t* __restrict__ ldbg, int32_t* __restrict__ fblk) {
  __shared__ __attribute__((aligned(16)))
      uint8_t win[(FL_T / 64) * (FC_WIN + 16)];      // one per wave
  __shared__ int64_t red[2 * (FL_T / 64) + 2];
  __shared__ int64_t s_next;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t n = stream_len(n_dev, n_cap);
  const int64_t ntiles = (n + FT_S - 1) / FT_S;
  if (ntiles == 0) {
    if (blockIdx.x == 0) {
      if (tid < 4) result[tid] = 0;
      if (tid == 0) *lastk = -1;
    }
    return;
  }
  const int64_t INF = INT64_MAX;
  const int64_t t_in = ldbg != nullptr ? wall_clock64() : 0;
  const FlCtx C{buf, n, ntiles, maxp, cap, sx, list, rcount, pre, rec_entry,
                rec_exit, rec_meta, base, bsum, result, lastk, stats, blist,
                lbw, cx, fblk, win, red};
  // the check over the grid (links, terminals, in-block counts; a launch of
  // its own until round 4), then a ticket: the last block to take one sees
  // every block's check (each releases it before its ticket) and goes on
  // alone; the others are done
  fl_check(C, mins, &g[FL_NB]);
  if (ldbg != nullptr && tid == 0 && blockIdx.x < FL_DBG_BLOCKS) {
    // (ZKMI_FS_DBG: every block's entry and check-done clocks, rows 1-4 of
    // fs_link's debug rows)
    ldbg[8 + 2 * blockIdx.x] = t_in;
    ldbg[8 + 2 * blockIdx.x + 1] = wall_clock64();
  }
  // the big repair (see FL_BIG_NOSPEC): barrier rounds over the grid, then
  // block 0 goes on as the last block does
  const bool big = (uint32_t)ld_agent((const int64_t*)&stats[LW_NOSPEC]) >
                   FL_BIG_NOSPEC;
  if (big) {
    unsigned long long* gb = (unsigned long long*)(stats + LW_BIG);
    bool ok = fl_sync(gb);
    for (int r = 0; r < FL_GROUNDS && ok; ++r)
      ok = fl_round(C, gb, r);
    if (blockIdx.x != 0) return;
    __syncthreads();
    if (tid == 0) {
      gb[2] = 0;
      for (int r = 0; r < FL_GROUNDS; ++r) gb[4 + 2 * r] = 0;
    }
  }
  // (the broken links — a frontier timeout, a garbage candidate, the ends
  // of a phantom chain's region — are all the last block's: an exact chase
  // runs on through a region of consistent-but-wrong links that no per-link
  // walk sees broken)
  __shared__ int s_last;
  __syncthreads();
  if (big) {
    if (tid == 0) s_last = 1;             // (block 0, after the rounds)
  } else if (tid == 0) {
    __threadfence();
    const unsigned long long a = __hip_atomic_fetch_add(
        &g[0], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    const int last = a + 1 == gridDim.x;
    // the ticket back to zero for the next scan of this workspace
    if (last)
      __hip_atomic_store(&g[0], 0ull, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  // the minima and the broken-link count (fs_rows clears them for the next
  // scan of this workspace)
  const uint64_t mb0 = ld_agent((const int64_t*)&mins[0]);
  const uint64_t mt0 = ld_agent((const int64_t*)&mins[1]);
  const unsigned long long nb0 = __hip_atomic_load(
      &g[FL_NB], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int64_t fb0 = mb0 ? ntiles - (int64_t)mb0 : INF;
  const int64_t ft0 = mt0 ? ntiles - (int64_t)mt0 : INF;
  if (!big && (fb0 == INF || fb0 > ft0)) {
    // no broken link before the first terminal: the row bases are bsum's
    // block offsets + the check's in-block bases
    if (ldbg != nullptr && tid == 0) ldbg[40] = wall_clock64();
    fl_bases(C, ft0);
    if (ldbg != nullptr && tid == 0) ldbg[41] = wall_clock64();
    return;
  }
  __shared__ uint32_t dirty[FL_DB / 32];
  __shared__ int s_ovf;
  FlChase ch{dirty, &s_ovf, stats, ldbg};
  for (int i = tid; i < FL_DB / 32; i += FL_T) dirty[i] = 0;
  if (tid == 0) s_ovf = 0;
  __syncthreads();
  const bool clk = ldbg != nullptr && tid == 0;
  // (ZKMI_FS_DBG: [5] the last block's start, [4] the end | path << 56:
  // 1 chases, 2 count scan after rounds, 3 tail)
  if (clk) ldbg[5] = t_in;
  int64_t from = 1, ft = INF;
  int64_t nb = (int64_t)nb0;
  // repair rounds of this block: a handful of broken links are chased (the
  // usual repair: one pass, then only the count blocks it touched are
  // re-counted); many are re-walked in parallel, one wave a link; after
  // each, the links still broken are listed again.  What the rounds leave
  // goes to the tail.
  bool changed = big;          // records changed beyond the chases' dirty
  if (!big && nb > (int64_t)FL_SMALL && fb0 != INF) {
    // many broken links: first ONE exact chase from the leftmost, wave 0,
    // through fs_tile's candidate exits 64 tiles a batch.  A stream whose
    // every frame carries a phantom chain of the frame's own period (SET_DATA
    // replies of version 84: both chains survive every tile, about half the
    // tiles speculate the phantom) is settled by it in one pass of lookups
    // (ms) where the rounds walked every broken tile (84 ms a scan).  Its
    // walks are budgeted: on a stream whose entries are not candidates
    // (dense payload words) it stops early and the rounds walk in parallel
    // (profiles/r5_fs_link_ab.md).  Not after the grid's big repair.
    if (wv == 0) {
      bool term = false;
      uint32_t walked = 0;
      const int64_t kend = fl_chase_run(C, win, ch, fb0, true, term, walked,
                                        FL_CHASE_WALKS);
      (void)kend;
      if (lane == 0) {
        if (walked) fc_stat(stats, 2, walked);
        fc_stat(stats, 3, 1);
      }
    }
    __syncthreads();
    changed = true;
  }
  for (int round = 0; round < FL_BROUNDS; ++round) {
    if (changed) {
      int64_t fbv, ftv;
      nb = fl_list_broken(C, fbv, ftv);
      if (fbv == INF || fbv > ftv) {
        fl_count_scan(C, ftv);
        if (clk) ldbg[4] = wall_clock64() | (2ll << 56);
        return;
      }
    }
    if (nb <= (int64_t)FL_SMALL && (ntiles + FK_T - 1) / FK_T <= FL_DB) {
      // ---- a handful of broken links: chases, then every link checked ---
      if (clk && round == 0) ldbg[0] = wall_clock64();
      const bool settled = fl_chase(C, (int)nb, ch);
      if (clk && round == 0) ldbg[1] = ldbg[2] = wall_clock64();
      // a chase only vouches for the links it saw
      int64_t fbv, ftv;
      fl_links(C, 1, fbv, ftv);
      if (clk && round == 0) ldbg[3] = wall_clock64();
      if (settled && (fbv == INF || fbv > ftv)) {
        if (changed) {
          // (tiles re-walked in rounds are not in the chases' dirty set)
          fl_count_scan(C, ftv);
          if (clk) ldbg[4] = wall_clock64() | (2ll << 56);
          return;
        }
        fl_chase_recount(C, ch);
        fl_bases(C, ftv);
        if (clk) ldbg[4] = wall_clock64() | (1ll << 56);
        return;
      }
      if (!settled) break;              // the lists outgrew LDS: the tail
    } else {
      const uint32_t w = fl_local_round(C, (int)nb);
      if (lane == 0 && w) fc_stat(stats, 2, w);
      if (tid == 0) fc_stat(stats, 3, 1);
      __syncthreads();
    }
    changed = true;
  }
  // ---- the tail: exact chases from the leftmost broken link, until every
  // live link holds; then the count scan ------------------------------------
  for (;;) {
    int64_t fb, fterm;
    fl_links(C, from, fb, fterm);
    // terminals before from - 1 were found in an earlier pass of this loop
    // (links before `from` hold)
    if (fb == INF || fb > fterm) {          // every live link holds
      ft = fterm;
      break;
    }
    if (wv == 0) {
      // the leftmost broken link has the exact entry (the exit before it):
      // the chase settles tile fb at least (looked up or walked)
      bool term = false;
      uint32_t walked = 0;
      const int64_t kend = fl_chase_run(C, win, ch, fb, true, term, walked);
      if (lane == 0) {
        // (kend < fb: nothing written, which the records before fb rule out;
        // the scan then stops before tile fb rather than loop)
        s_next = kend < fb ? -fb : kend + 1;
        if (walked) fc_stat(stats, 2, walked);
        fc_stat(stats, 3, 1);
      }
    }
    __syncthreads();
    from = s_next;
    __syncthreads();
    if (from < 0) {
      ft = -from - 1;
      break;
    }
  }
  fl_count_scan(C, ft);
  if (clk) ldbg[4] = wall_clock64() | (3ll << 56);
}

int link_launch(const uint8_t* buf, const int64_t* n_dev, int64_t n_cap,
                int64_t maxp, const FsWs& ws, int64_t cap, int64_t* result,
                int64_t* ldbg, hipStream_t st) {
  FsTail* t = ws.tail;
  fs_link<<<FL_BLOCKS, FL_T, 0, st>>>(
      buf, n_dev, n_cap, maxp, ws.sx, ws.list, ws.rcnt, ws.pre, ws.rent,
      ws.rexit, ws.rmeta, ws.base, cap, result, (uint64_t*)t, ws.blist,
      ws.bsum, t->mins, &t->lastk, t->grid, ws.lbw, ws.cx, ldbg, ws.fblk);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace zk
