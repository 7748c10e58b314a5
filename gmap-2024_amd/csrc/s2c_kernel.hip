// s2c_kernel.hip -- CDNA4 (gfx950) kernel for GMAP's stage-2 chaining: what
// Stage2_compute (stage2.c:6325) does with the seeding that oi_kernel / oi_map_kernel leave in HBM.
//
// Reference semantics restated (paths under the reference tree's src/; GMAP's arguments, gmap.c:1208:
// localp, skip_repetitive_p, proceed_pctcoverage 0.3, favor_right_p false, max_nalignments 10; no SNPs,
// STANDARD mode; cross-species canonical scoring in the sweep's canonical variant, s2b_canon_kernel):
//   Diag_update_coverage          diag.c:216
//   the proceed test              stage2.c:6521-6531
//   Diag_compute_bounds           diag.c:597 (assign_scores :521, compute_dominance :427,
//                                 keep_center_diagonal :493, the minactive / maxactive lines)
//   align_compute_scores_lookback stage2.c:3667 with score_querypos_lookback_one / _mult (:1073 / :1470),
//                                 revise_active_lookback (:2956) and the grand lookback (:3983-4020)
//   get_cells_fwd                 stage2.c:3437, the path loop of align_compute_lookback (:4465-4515)
//   traceback_one                 stage2.c:4140
//   convert_to_nucleotides        stage2.c:5334
//   Stage2_filter_unique          stage2.c:6013 (stage2_cmp, stage2pairs_overlap_p)
// glibc's qsort is a stable merge sort on this image, so every sort here is stable.
//
// Design.  One wave per Stage2_compute call.  The wave does the data-parallel parts: coverage and
// diagonal depth (difference arrays + wave prefix scans), the minactive / maxactive lines (a segment
// list, each segment filled by all lanes), the per-hit arrays (of every query position the hits inside
// [minactive, maxactive], laid out contiguously by a prefix scan of their counts, so a link is one index;
// the first position with hits keeps all of them: s2a_kernel), the cell selection (a
// max-reduction, a compaction of the cells within FINAL_SCORE_TOLERANCE of the best, group maxima and
// ranks by lane), the duplicate filter and convert_to_nucleotides (per path entry record counts, a
// prefix scan, every record written in place in list order).  The querypos sweep of
// align_compute_scores_lookback and the pointer chase of traceback_one are inherently sequential; they
// run on lane 0 over the problem's L2-resident link arrays.  Scratch and outputs come from batch-wide
// pools (one atomic per problem); a problem that does not fit reports kS2Overflow and the host reruns
// the batch with larger pools.
#include <cstdlib>

#include "dp_device.h"
#include "canon_device.h"
#include <climits>

namespace gmapdp {

constexpr int kS2K = 8;                 // indexsize of GMAP's major oligoindex
constexpr int kS2EqualNotSplicing = 9;  // EQUAL_DISTANCE_NOT_SPLICING
constexpr int kS2EnoughConsec = 32;     // ENOUGH_CONSECUTIVE
constexpr int kS2GreedyConsec = 100;    // GREEDY_NCONSECUTIVE
constexpr int kS2ExonDefn = 30;         // EXON_DEFN
constexpr int kS2MinTerminal = 8;       // MIN_TERMINAL_NCONSECUTIVE
constexpr int kS2MaxNactive = 100;      // MAX_NACTIVE
constexpr int kS2MaxSkipped = 3;        // MAX_SKIPPED
constexpr int kS2ScoreRestrict = 10;    // SCORE_FOR_RESTRICT
constexpr int kS2TenThousand = 8192;    // TEN_THOUSAND
constexpr int kS2FinalTolerance = 20;   // FINAL_SCORE_TOLERANCE
constexpr int kS2MaxNalignments = 10;   // gmap.c:142
constexpr int kS2Sufflookback = 60, kS2Nsufflookback = 5;  // gmap.c:269-270
constexpr int kS2ExtraBounds = 20;      // diag.c:14
constexpr int kS2cCap = 4096;           // hits of s2c's LDS link table (8 B each, 32 KB: 5 waves per CU)
// Which of s2c's two launches takes a call: the one with the LDS link table when it holds the call's hits
// and a query position fits 16 bits.  seeded: the seeding's hit count, laid: the hits s2a laid out (<= seeded).
// s2a (zeroed records or not) and both s2c launches evaluate this alike.
#ifndef GMAPDP_S2C_CLASS_LAID
#define GMAPDP_S2C_CLASS_LAID 0  // 1: by the laid-out count (variants: make variant DEFS=...)
#endif
__host__ __device__ inline bool s2c_lds_class(int seeded, int laid, int nq) {
  return (GMAPDP_S2C_CLASS_LAID ? laid : seeded) <= kS2cCap && nq <= 65536;
}

// Phase timing (tools/oi_timing.py s2; the GMAPDP_OI_TIMING variant of the library only)
#ifdef GMAPDP_OI_TIMING
__device__ unsigned long long g_s2_marks[2][16];
__device__ unsigned int g_s2_wave[3][16384];  // per call (< 16384): sweep duration (wall-clock ticks), positions, hits
// s2_one's parts, summed over the waves (wall-clock ticks): adjacent hit, prefetch, fast window, multi
// windows, the entry-by-entry tail, and their call counts
__device__ unsigned long long g_s2_sub[2][8];
#define S2_SUB_DECL() unsigned long long _sub_t0 = 0
#define S2_SUB_T0() (_sub_t0 = wall_clock64())
#define S2_SUB(k) (W.sub[k] += wall_clock64() - _sub_t0, W.subn[k]++)
#define S2_MARK(k)                                                  \
  do {                                                              \
    if (threadIdx.x == 0) {                                         \
      atomicAdd(&g_s2_marks[0][k], (unsigned long long)wall_clock64()); \
      atomicAdd(&g_s2_marks[1][k], 1ull);                           \
    }                                                               \
  } while (0)
#define S2_COUNT(k, v)                                             \
  do {                                                              \
    if (threadIdx.x == 0) atomicAdd(&g_s2_marks[0][k], (unsigned long long)(v)); \
  } while (0)
#else
#define S2_MARK(k) \
  do {             \
  } while (0)
#define S2_COUNT(k, v) \
  do {                 \
  } while (0)
#define S2_SUB_DECL() (void)0
#define S2_SUB_T0() (void)0
#define S2_SUB(k) (void)0
#endif

// result status
constexpr int kS2NoPositions = 0, kS2Coverage = 1, kS2Chained = 2, kS2Overflow = -2, kS2Domain = -3;

// struct Link_T (stage2.c:363) + fwd_scores, one per (querypos, hit).  Written by the sweep (s2b) for every
// hit it scores; the hits it never scores keep score 0 in the compact score array (4 B per hit, zeroed by
// s2a with the chrpos array), which is all that get_cells' scan and the sweep read of them.  Only the hits
// the chaining can touch are laid out at all (s2a_kernel: about 1 900 of the ~8 200 a 214-kb window seeds
// per call).  Calls of the LDS link table's class (its loader reads every record) get zeroed records.
// 16 B, one store: the score lives only in the score array, the chrpos in the maps array, and the link is
// the predecessor's hit index within the call (-1: none; off[] ascends, so the hit index gives back the
// query position, s2_hit_pos / s2_hit_pos_wave).
struct __attribute__((aligned(16))) S2Hit {
  int consec, root, tracei, pred;
};
struct S2Diag {  // struct Diag_T (diagdef.h)
  uint32_t diagonal;
  int querystart, queryend, nconsecutive, dominatedp, pad_;
  double score;
};
struct S2Path {
  int cell;          // end cell (hit index)
  int n;             // path entries after the 3'-end pruning
  uint32_t start, end;  // genomepos of the first and last pair of the converted list
};
struct S2Scratch {
  size_t diff, run, off, minact, maxact, first, proc, diags, ord, tmp, hits, maps, sc, cand, keep, paths, pq, ph, lh,
      sbuf, total;
  int sortn;  // power of two >= every sorted array
};
__host__ __device__ inline int s2_pow2(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}
__host__ __device__ inline S2Scratch s2_scratch(int ql, int T, int nd) {
  S2Scratch s;
  const size_t Q = (size_t)ql + 1, D = (size_t)(nd > 0 ? nd : 1), H = (size_t)(T > 0 ? T : 1);
  s.diff = 0;
  s.run = align16(s.diff + 4 * Q);
  s.off = align16(s.run + 8 * Q);
  s.minact = align16(s.off + 4 * Q);
  s.maxact = align16(s.minact + 4 * Q);
  s.first = align16(s.maxact + 4 * Q);
  s.proc = align16(s.first + 4 * Q);
  s.diags = align16(s.proc + 4 * Q);
  s.ord = align16(s.diags + sizeof(S2Diag) * D);
  s.tmp = align16(s.ord + 4 * D);
  s.hits = align16(s.tmp + 4 * D);
  s.maps = align16(s.hits + sizeof(S2Hit) * H);  // the hits' chrpos, 4 B each (the sweep, the path walk)
  s.sc = align16(s.maps + 4 * H);                // the hits' scores, 4 B each (fwd_scores; get_cells' scan)
  s.cand = align16(s.sc + 4 * H);
  s.keep = align16(s.cand + 4 * H);
  s.paths = align16(s.keep + 4 * H);
  s.pq = align16(s.paths + sizeof(S2Path) * H);
  s.ph = align16(s.pq + 4 * Q);
  s.lh = align16(s.ph + 4 * Q);  // the active range [low, high) of the first position with hits (s2a_kernel)
  s.sortn = s2_pow2((int)(H > D ? H : D));
  s.sbuf = align16(s.lh + 8 * Q);
  s.total = align16(s.sbuf + 4 * (size_t)s.sortn);
  return s;
}

// ---- wave primitives ----
__device__ __forceinline__ int wave_incl_sum(int x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}
__device__ __forceinline__ int wave_incl_max(int x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x = max(x, y);
  }
  return x;
}
__device__ __forceinline__ int wave_max_i(int x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = max(x, __shfl_xor(x, off, 64));
  return x;
}
__device__ __forceinline__ int wave_sum_i(int x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ void wave_sync() { __syncthreads(); }  // one wave per block: waitcnt + barrier

// Stable sort of in[0..n) into out[0..n) by `less` (a strict weak order on the values): a bitonic
// sort of the positions 0..n-1 in sbuf (padded with -1 = +infinity to a power of two), ties broken
// by position, which is the order a stable merge sort (glibc qsort) leaves.
template <class Less>
__device__ void wave_sort(int lane, int n, const int* in, int* out, int* sbuf, Less less) {
  if (n <= 0) return;
  const int NN = s2_pow2(n);
  for (int i = lane; i < NN; i += 64) sbuf[i] = i < n ? i : -1;
  wave_sync();
  auto lt = [&](int x, int y) {  // positions; -1 sorts last
    if (x < 0) return false;
    if (y < 0) return true;
    const int vx = in[x], vy = in[y];
    if (less(vx, vy)) return true;
    if (less(vy, vx)) return false;
    return x < y;
  };
  for (int size = 2; size <= NN; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = lane; i < NN; i += 64) {
        const int j = i ^ stride;
        if (j > i) {
          const int a = sbuf[i], b = sbuf[j];
          const bool up = (i & size) == 0;
          if (up ? lt(b, a) : lt(a, b)) {
            sbuf[i] = b;
            sbuf[j] = a;
          }
        }
      }
      wave_sync();
    }
  }
  for (int i = lane; i < n; i += 64) out[i] = in[sbuf[i]];
  wave_sync();
}

// fill dst[a..b] (inclusive) with f(q) by all lanes
template <class F>
__device__ __forceinline__ void fill_range(int lane, uint32_t* dst, int a, int b, F f) {
  for (int q = a + lane; q <= b; q += 64) dst[q] = f(q);
}

struct S2Best {  // pp: the predecessor's query position (-1: none), ph: its hit index within the call
  int consec, root, pp, ph, score, tracei;
};
// The link is wave-uniform by construction (every update comes from readlane/readfirstlane values);
// restating that keeps it in SGPRs, so the tests on it are scalar branches rather than exec-mask ones.
__device__ __forceinline__ void s2_uniform(S2Best& b) {
  b.consec = __builtin_amdgcn_readfirstlane(b.consec);
  b.root = __builtin_amdgcn_readfirstlane(b.root);
  b.pp = __builtin_amdgcn_readfirstlane(b.pp);
  b.ph = __builtin_amdgcn_readfirstlane(b.ph);
  b.score = __builtin_amdgcn_readfirstlane(b.score);
  b.tracei = __builtin_amdgcn_readfirstlane(b.tracei);
}

// ---- align_compute_scores_lookback, wave-uniform ----
// Every lane runs the sweep's control flow; per-position metadata is prefetched 64 query positions at
// a time (one coalesced load each, then readlane), the active hits of the most recently processed
// query positions sit in an LDS ring, and one processed position's ranges 0-4 are evaluated across
// lanes: the range boundaries are ballots (the active hits ascend in chrpos, so every range
// condition but range 0's is monotone), the best link of a range is a wave max plus the first lane
// holding it (the reference's strict '>' keeps the first maximum).  tracei values only ever meet in
// equality tests (range 0), so a fresh value per improvement event replaces the reference's
// per-improvement counter without changing any decision.
constexpr int kS2Ring = 128;
// processed entries whose metadata stays in LDS: every lookback stays within the newest 128 (entries
// sit at distinct query positions, so donep ends a walk by entry 73; the _mult bounds stop at 128)
constexpr int kS2Meta = 128;
constexpr int kS2Pref = 64;  // entries S2Pref holds (one per lane)
struct S2Ring {
  uint32_t map[kS2Ring];
  int score[kS2Ring], consec[kS2Ring], tracei[kS2Ring], root[kS2Ring], hit[kS2Ring];
  int eq[kS2Meta], en[kS2Meta], eoff[kS2Meta], estart[kS2Meta];
};
// the sweep's LDS (one wave per workgroup): ds_* instructions rather than flat ones
static __shared__ S2Ring s2_ring;
static __shared__ int s2_fr[128];
static __shared__ int s2_head[64];  // s2_dloop_multi: the entry whose hits start at each lane

// a value every lane holds (loaded from a uniform address) as a scalar: scalar branches
__device__ __forceinline__ int s2_u(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t s2_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct S2HV {  // one hit's link state; hit: its index within the call (off[q] + its index at q), here and in
  uint32_t map;  // the ring, so a link to it is stored as it stands
  int score, consec, tracei, root, hit;
};
struct S2E {  // a processed query position: its active hits
  int q, n, start, offq;
  bool inring;
};
// forms of the range-2 evaluation: s2_eval's one-hit scalar form and its 64-lane chunks, s2_eval1, the
// one-wave-step windows s2_dloop_fast and s2_dloop_multi
constexpr int kS2FormScalar = 0, kS2FormChunk = 1, kS2FormEval1 = 2, kS2FormFast = 3, kS2FormMulti = 4;
// the canonical sweeps' counters since the last gmapdp_debug_canon_counters: [0..4] candidates per form from
// score_querypos_lookback_one's walk, [5..6] s2_eval's scalar form / chunks called from _mult, [7] shifts
// whose MaxEnt models were evaluated
__device__ unsigned long long g_s2_canon[8];
// kCanon: the cross-species variant of the sweep (GMAPDP_S2_CANONICAL_MIDDLE): range 2 takes
// NON_CANONICAL_PENALTY_MIDDLE off every link that canonical_link (canon_device.h) declines
// kLocal / kMiddle / kSkip: align_compute_lookback's localp, middlep and skip_repetitive_p.  Stage2_compute
// passes true / true / true; Stage2_compute_one true / true / false; Stage2_compute_ends false / false / false
// (DevStage2Problem.kind, one per launch).  Where the sweep depends on them:
//   kLocal   a hit without a predecessor scores indexsize; else it keeps the search's 0 (stage2.c:1445-1451,
//            :1551-1556, :1993-1999).  The shortcuts below never involve such a hit's score: the run on the last
//            entry's diagonal links every member to a predecessor, and the one-wave windows (s2_dloop_fast /
//            _multi) only read hits that are active, i.e. scored above 0 under either setting.
//   kMiddle  else a position none of whose hits scored above 0 restarts every hit (:3955-3980): score and consec
//            indexsize, no link, tracei -1 -- a value range 0 compares like any other (last_tr starts at -1).
//   kSkip    the MAX_NACTIVE / MAX_SKIPPED branch (:3862-3887); without it every position goes through s2_one,
//            the <= 64-hit form or s2_mult by its hit count alone.
template <bool kC, bool kLocal = true, bool kMiddle = true, bool kSkip = true>
struct S2WT {
  static constexpr bool kCanon = kC;
  static constexpr bool kLocalp = kLocal, kMiddlep = kMiddle, kSkipRepetitive = kSkip;
  S2Hit* hits;
  const uint32_t* maps;  // chrpos per hit
  int* sc;               // score per hit (fwd_scores)
  const int* off;
  int* actn;       // per query position: number of active hits (firstactive != -1 <=> actn > 0)
  int* alist;      // active hits of q at alist[off[q] ...] (hit indices, ascending)
  int *pq, *pn, *poff, *pstart;  // per processed entry: q, active count, off[q], ring start
  int pushed, tracectr, splicingp, lane;
  uint32_t maxintronlen;
  // kCanon only: the genome, the MaxEnt tables and the call's strand and chromosome
  const uint32_t* blocks;
  const double* metab;
  uint64_t nwords, chroffset, chrhigh;
  int plusp;
  // kCanon only: range-2 candidates tested per form of the evaluation (per lane; kS2Form*), shifts whose
  // MaxEnt models were evaluated; summed into g_s2_canon at the sweep's end (gmapdp_debug_canon_counters)
  unsigned nform[5], nmult[2], nevals;
  int in_mult;
  // the range-2 score of the link from the hit at pp, qd query positions back (fs: without the penalty);
  // uniform: every lane evaluates the same candidate (counted once)
  __device__ __forceinline__ int canon(int fs, uint32_t pp, uint32_t position, int qd, int form, bool uniform) {
    if constexpr (kC) {
      unsigned ev = 0;
      if (!canonical_hit_link(blocks, nwords, metab, pp, position, qd, plusp != 0, chroffset, chrhigh, &ev))
        fs -= kCanonPenaltyMiddle;
      if (!uniform || lane == 0) {
        if (in_mult) form = kS2FormMulti + 1 + form;  // (s2_mult only calls s2_eval: forms 0 and 1)
        if (form < 5) nform[form]++;
        else if (form == 5) nmult[0]++;
        else nmult[1]++;
        nevals += ev;
      }
    }
    return fs;
  }
#ifdef GMAPDP_OI_TIMING
  unsigned long long n_cand = 0, n_fast = 0, n_slow = 0, n_multi = 0;  // candidates, fast/multi windows, slow evals
  unsigned long long n_runs = 0, n_runpos = 0, n_onepos = 0, n_multpos = 0;  // runs, their members, other positions
  unsigned long long sub[8] = {}, subn[8] = {};  // s2_one's parts (registers; flushed once per wave)
#define S2_TALLY(f, v) (W.f += (v))
#else
#define S2_TALLY(f, v) (void)0
#endif
};
using S2W = S2WT<false>;

__device__ __forceinline__ S2HV s2_bcast(const S2HV& v, int j) {
  S2HV u;
  u.map = (uint32_t)__builtin_amdgcn_readlane((int)v.map, j);
  u.score = __builtin_amdgcn_readlane(v.score, j);
  u.consec = __builtin_amdgcn_readlane(v.consec, j);
  u.tracei = __builtin_amdgcn_readlane(v.tracei, j);
  u.root = __builtin_amdgcn_readlane(v.root, j);
  u.hit = __builtin_amdgcn_readlane(v.hit, j);
  return u;
}

// an entry's hit outside the ring (rare): its own function so that the ring path's loads stay
// ds_* instructions instead of being merged into flat loads through a selected pointer
__device__ __attribute__((noinline)) S2HV s2_load_global(const S2Hit* hits, const uint32_t* maps, const int* sc,
                                                        const int* alist, int offq, int k) {
  S2HV v;
  const int h = offq + alist[offq + k];
  const S2Hit x = hits[h];
  v.map = maps[h];
  v.score = sc[h];
  v.consec = x.consec;
  v.tracei = x.tracei;
  v.root = x.root;
  v.hit = h;
  return v;
}

template <class SW>
__device__ __forceinline__ S2HV s2_load(const SW& W, const S2E& e, int k) {
  if (!e.inring) return s2_load_global(W.hits, W.maps, W.sc, W.alist, e.offq, k);  // (callers fence first)
  S2HV v;
  const int s = (e.start + k) & (kS2Ring - 1);
  v.map = s2_ring.map[s];
  v.score = s2_ring.score[s];
  v.consec = s2_ring.consec[s];
  v.tracei = s2_ring.tracei[s];
  v.root = s2_ring.root[s];
  v.hit = s2_ring.hit[s];
  return v;
}

template <class SW>
__device__ __forceinline__ S2E s2_mkentry(const SW& W, int q, int n, int offq, int start) {
  S2E e;
  e.q = q;
  e.n = n;
  e.offq = offq;
  e.start = start;
  e.inring = n <= kS2Ring && start >= W.pushed - kS2Ring;
  return e;
}

// Section A: from active index k_io, the first hit with map + qd >= position (k_io := it, or -1 when
// the list runs out); true when it sits exactly qd before position (its state in `out`)
template <class SW>
__device__ __forceinline__ bool s2_adj(const SW& W, const S2E& e, int& k_io, int qd, uint32_t position, S2HV& out) {
  if (k_io < 0) return false;
  if (e.n == 1 && e.inring) {  // one active hit (the common case): uniform LDS reads, no ballots
    const int sl = e.start & (kS2Ring - 1);
    const uint32_t mp = s2_u(s2_ring.map[sl]);
    if (!(mp + (uint32_t)qd >= position)) {
      k_io = -1;
      return false;
    }
    k_io = 0;
    if (mp + (uint32_t)qd != position) return false;
    out.map = mp;
    out.score = s2_u(s2_ring.score[sl]);
    out.consec = s2_u(s2_ring.consec[sl]);
    out.tracei = s2_u(s2_ring.tracei[sl]);
    out.root = s2_u(s2_ring.root[sl]);
    out.hit = s2_u(s2_ring.hit[sl]);
    return true;
  }
  if (!e.inring) wave_sync();
  for (int c0 = k_io; c0 < e.n; c0 += 64) {
    const int k = c0 + W.lane;
    const bool valid = k < e.n;
    S2HV v = {};
    if (valid) v = s2_load(W, e, k);
    const uint64_t m = ballot(valid && v.map + (uint32_t)qd >= position);
    if (m) {
      const int j = __ffsll((long long)m) - 1;
      k_io = c0 + j;
      const S2HV u = s2_bcast(v, j);
      if (u.map + (uint32_t)qd == position) {
        out = u;
        return true;
      }
      return false;
    }
  }
  k_io = -1;
  return false;
}

// Ranges 0-4 of score_querypos_lookback_one/_mult against processed entry e from active index start;
// returns the index where the range-0/1 skipping stopped (the _mult frontier), -1 when the list ran out.
template <class SW>
__device__ __forceinline__ int s2_eval(SW& W, const S2E& e, int start, int q, uint32_t position, int& last_tr, S2Best& b,
                       bool range1) {
  const int qd = q - e.q, credit = -qd / kS2K;
  if (e.n == 1 && e.inring && start == 0) {  // one active hit: the ranges in scalar form
    const int sl = e.start & (kS2Ring - 1);
    const int tr = s2_u(s2_ring.tracei[sl]);
    if (tr == last_tr) return -1;  // range 0 (nothing left for the frontier either)
    last_tr = tr;
    const uint32_t mp = s2_u(s2_ring.map[sl]);
    if (range1 && mp + W.maxintronlen + (uint32_t)qd <= position) return -1;
    if (mp + (uint32_t)kS2EqualNotSplicing + (uint32_t)qd < position) {
      const int diff = (int)(position - mp) - qd;
      const int fs = W.canon(
          s2_u(s2_ring.score[sl]) + credit - (W.splicingp ? (diff / kS2TenThousand + 1) : (diff + 1)), mp, position, qd,
          kS2FormScalar, true);
      if (fs > b.score) {
        b.consec = 0;
        b.root = s2_u(s2_ring.root[sl]);
        b.score = fs;
        b.pp = e.q;
        b.ph = s2_u(s2_ring.hit[sl]);
        b.tracei = ++W.tracectr;
      }
    } else if (mp + (uint32_t)kS2K <= position) {
      const int fs = s2_u(s2_ring.score[sl]) + 1;
      if (fs > b.score) {
        const int g = (int)(position - mp);
        const int diff = g > qd ? g - qd : qd - g;
        b.consec = (diff <= 0) ? s2_u(s2_ring.consec[sl]) + qd : 0;
        b.root = s2_u(s2_ring.root[sl]);
        b.score = fs;
        b.pp = e.q;
        b.ph = s2_u(s2_ring.hit[sl]);
        b.tracei = tr;
      }
    }
    return 0;
  }
  int state = 0, frontier = -1;  // 0 range 0, 1 range 1, 2 range 2, 4 ranges 3-4, 5 done
  if (!e.inring) wave_sync();
  for (int c0 = start; c0 < e.n && state != 5; c0 += 64) {
    const int k = c0 + W.lane;
    const bool valid = k < e.n;
    S2HV v = {};
    if (valid) v = s2_load(W, e, k);
    int cs = 0;  // first lane of the current range in this chunk
    if (state == 0) {
      const uint64_t m = ballot(valid && v.tracei != last_tr);
      if (!m) continue;  // every hit of this chunk carries last_tr
      cs = __ffsll((long long)m) - 1;
      last_tr = __builtin_amdgcn_readlane(v.tracei, cs);
      state = range1 ? 1 : 2;
      if (!range1) frontier = c0 + cs;
    }
    if (state == 1) {
      const uint64_t m = ballot(valid && W.lane >= cs && !(v.map + W.maxintronlen + (uint32_t)qd <= position));
      if (!m) continue;
      cs = __ffsll((long long)m) - 1;
      frontier = c0 + cs;
      state = 2;
    }
    if (state == 2) {
      const bool in2 = valid && W.lane >= cs && v.map + (uint32_t)kS2EqualNotSplicing + (uint32_t)qd < position;
      const uint64_t m = ballot(in2);
      int fs = INT_MIN;
      if (in2) {
        const int diff = (int)(position - v.map) - qd;
        fs = W.canon(v.score + credit - (W.splicingp ? (diff / kS2TenThousand + 1) : (diff + 1)), v.map, position, qd,
                     kS2FormChunk, false);
      }
      const int mx = wave_max_i(fs);
      if (m && mx > b.score) {
        const int j = __ffsll((long long)ballot(in2 && fs == mx)) - 1;
        const S2HV u = s2_bcast(v, j);
        b.consec = 0;  // diff > EQUAL_DISTANCE_NOT_SPLICING
        b.root = u.root;
        b.score = mx;
        b.pp = e.q;
        b.ph = u.hit;
        b.tracei = ++W.tracectr;
      }
      const uint64_t rest = ballot(valid && W.lane >= cs) & ~m;
      if (!rest) continue;  // the chunk ended inside range 2
      cs = __ffsll((long long)rest) - 1;
      state = 4;
    }
    if (state == 4) {
      const bool in4 = valid && W.lane >= cs && v.map + (uint32_t)kS2K <= position;
      const uint64_t m = ballot(in4);
      const int fs = in4 ? v.score + 1 : INT_MIN;
      const int mx = wave_max_i(fs);
      if (m && mx > b.score) {
        const int j = __ffsll((long long)ballot(in4 && fs == mx)) - 1;
        const S2HV u = s2_bcast(v, j);
        const int g = (int)(position - u.map);
        const int diff = g > qd ? g - qd : qd - g;
        b.consec = (diff <= 0) ? u.consec + qd : 0;
        b.root = u.root;
        b.score = mx;
        b.pp = e.q;
        b.ph = u.hit;
        b.tracei = u.tracei;
      }
      if (ballot(valid && W.lane >= cs) & ~m) state = 5;
    }
  }
  return frontier;
}

// the kk-th newest processed entry (kk < kS2Meta) from the LDS metadata ring
struct S2EntryCache {
  template <class SW>
  __device__ __forceinline__ S2E get(const SW& W, int np, int kk) {
    const int s = (np - 1 - kk) & (kS2Meta - 1);
    return s2_mkentry(W, s2_u(s2_ring.eq[s]), s2_u(s2_ring.en[s]), s2_u(s2_ring.eoff[s]), s2_u(s2_ring.estart[s]));
  }
};

// The 64 newest processed entries, one per lane (metadata, and the hit of one-hit entries in the
// ring), loaded once per lookback so the sequential walk over them reads registers.
struct S2Pref {
  int q = 0, n = 0, off = 0, start = 0;
  S2HV h = {};
  template <class SW>
  __device__ __forceinline__ void load(const SW& W, int np, int base = 0) {
    const int k = np - 1 - base - W.lane;  // entry base + lane (0: the newest)
    q = n = off = start = 0;
    h = {};
    if (k >= 0) {
      const int s = k & (kS2Meta - 1);
      q = s2_ring.eq[s];
      n = s2_ring.en[s];
      off = s2_ring.eoff[s];
      start = s2_ring.estart[s];
      if (n == 1 && start >= W.pushed - kS2Ring) {
        const int sl = start & (kS2Ring - 1);
        h.map = s2_ring.map[sl];
        h.score = s2_ring.score[sl];
        h.consec = s2_ring.consec[sl];
        h.tracei = s2_ring.tracei[sl];
        h.root = s2_ring.root[sl];
        h.hit = s2_ring.hit[sl];
      }
    }
  }
  template <class SW>
  __device__ __forceinline__ S2E entry(const SW& W, int kk) const {
    return s2_mkentry(W, __builtin_amdgcn_readlane(q, kk), __builtin_amdgcn_readlane(n, kk),
                      __builtin_amdgcn_readlane(off, kk), __builtin_amdgcn_readlane(start, kk));
  }
};

// ranges 0-4 against a processed entry with a single active hit u (scalar); the frontier is 0 or -1
template <class SW>
__device__ __forceinline__ int s2_eval1(SW& W, int eq, const S2HV& u, int q, uint32_t position, int& last_tr,
                                        S2Best& b, bool range1) {
  const int qd = q - eq;
  if (u.tracei == last_tr) return -1;
  last_tr = u.tracei;
  if (range1 && u.map + W.maxintronlen + (uint32_t)qd <= position) return -1;
  if (u.map + (uint32_t)kS2EqualNotSplicing + (uint32_t)qd < position) {
    const int diff = (int)(position - u.map) - qd;
    const int fs =
        W.canon(u.score + (-qd / kS2K) - (W.splicingp ? (diff / kS2TenThousand + 1) : (diff + 1)), u.map, position, qd,
                kS2FormEval1, true);
    if (fs > b.score) {
      b.consec = 0;
      b.root = u.root;
      b.score = fs;
      b.pp = eq;
      b.ph = u.hit;
      b.tracei = ++W.tracectr;
    }
  } else if (u.map + (uint32_t)kS2K <= position) {
    const int fs = u.score + 1;
    if (fs > b.score) {
      const int g = (int)(position - u.map);
      const int diff = g > qd ? g - qd : qd - g;
      b.consec = (diff <= 0) ? u.consec + qd : 0;
      b.root = u.root;
      b.score = fs;
      b.pp = eq;
      b.ph = u.hit;
      b.tracei = u.tracei;
    }
  }
  return 0;
}

// one processed entry of a lookback: prefetched (kk < 64) or fetched
template <class SW>
__device__ __forceinline__ int s2_entry_eval(SW& W, const S2Pref& pf, S2EntryCache& ec, int np, int kk, int start,
                                             int q, uint32_t position, int& last_tr, S2Best& b, bool range1,
                                             int* qd_out) {
  const S2E e = kk < kS2Pref ? pf.entry(W, kk) : ec.get(W, np, kk);
  S2_TALLY(n_slow, 1);
  *qd_out = q - e.q;
  if (e.n <= 0 || start < 0) return -1;
  if (kk < kS2Pref && e.n == 1 && e.inring && start == 0)
    return s2_eval1(W, e.q, s2_bcast(pf.h, kk), q, position, last_tr, b, range1);
  return s2_eval(W, e, start, q, position, last_tr, b, range1);
}

// Section D over the newest processed entries [0, kmax] in one wave step, when every entry that would
// be evaluated holds a single active hit in the ring (the common case).  For such entries range 0
// leaves last_tr = the entry's tracei whether it skips or not, so "skipped" is "same tracei as the
// nearest earlier evaluated entry" (a ballot and one lane shuffle); only the remaining candidates are
// walked in order, and only they can change the link or end the loop (consec >= ENOUGH_CONSECUTIVE).
// use_f: _mult's per-entry frontiers (lane kk holds f, 0 or -1), updated for the visited entries.
// Windows past 64 entries: the first 64 here, then (return 2) the walk goes on from entry 64 with
// last_tr = lt.  Returns 0 (nothing done) when the window holds another kind of entry, 1 when done.
template <class SW>
__device__ __forceinline__ int s2_dloop_fast(SW& W, const S2Pref& pf, int np, int kmax, int q, uint32_t position,
                                             S2Best& b, bool range1, bool use_f, int& f, int& lt) {
  const int kend = kmax < 63 ? kmax : 63;
  const int kk = W.lane;
  const bool inw = kk <= kend && kk < np;
  const bool valid = inw && pf.n > 0 && (!use_f || f != -1);
  const bool simple = pf.n == 1 && pf.start >= W.pushed - kS2Ring;
  if (ballot(valid && !simple)) return 0;
  s2_uniform(b);
  if (b.consec >= kS2EnoughConsec) return 1;
  const uint64_t V = ballot(valid);
  const uint64_t below = kk ? (V & ((1ull << kk) - 1ull)) : 0ull;
  const int prev = below ? 63 - __clzll((long long)below) : 0;
  const int ptr = __shfl(pf.h.tracei, prev, 64);
  const int last_tr = below ? ptr : -1;
  const int qd = q - pf.q;
  const bool skip = valid && pf.h.tracei == last_tr;
  const bool r1skip = valid && !skip && range1 && pf.h.map + W.maxintronlen + (uint32_t)qd <= position;
  int kind = 0, fs = 0;
  if (valid && !skip && !r1skip) {
    if (pf.h.map + (uint32_t)kS2EqualNotSplicing + (uint32_t)qd < position) {
      const int diff = (int)(position - pf.h.map) - qd;
      kind = 2;
      fs = W.canon(pf.h.score + (-qd / kS2K) - (W.splicingp ? (diff / kS2TenThousand + 1) : (diff + 1)), pf.h.map,
                   position, qd, kS2FormFast, false);
    } else if (pf.h.map + (uint32_t)kS2K <= position) {
      kind = 4;
      fs = pf.h.score + 1;
    }
  }
  // The walk over the candidates in entry order keeps the first strictly better score each time and stops
  // after an update whose consec reaches ENOUGH_CONSECUTIVE: the updates are the records of a prefix max
  // seeded with the current score, the walk ends at the first record with such a consec, else the last
  // record wins (one wave scan instead of a scalar step per candidate).
  int cons = 0;
  if (kind == 4) {
    const int g = (int)(position - pf.h.map);
    const int diff = g > qd ? g - qd : qd - g;
    cons = (diff <= 0) ? pf.h.consec + qd : 0;
  }
  const int fsv = kind != 0 ? fs : INT_MIN;
  int pm = __shfl_up(wave_incl_max(fsv, kk), 1, 64);
  if (kk == 0) pm = INT_MIN;
  pm = max(pm, b.score);
  const bool rec = kind != 0 && fsv > pm;
  const uint64_t R = ballot(rec);
  const uint64_t S = ballot(rec && cons >= kS2EnoughConsec);
  S2_TALLY(n_fast, 1);
  S2_TALLY(n_cand, __popcll(R));
  int w = -1;
  if (S) w = __ffsll((long long)S) - 1;
  else if (R) w = 63 - __clzll((long long)R);
  if (w >= 0) {
    b.score = __builtin_amdgcn_readlane(fs, w);
    b.consec = __builtin_amdgcn_readlane(cons, w);
    b.root = __builtin_amdgcn_readlane(pf.h.root, w);
    b.pp = __builtin_amdgcn_readlane(pf.q, w);
    b.ph = __builtin_amdgcn_readlane(pf.h.hit, w);
    b.tracei = __builtin_amdgcn_readlane(kind, w) == 2 ? ++W.tracectr : __builtin_amdgcn_readlane(pf.h.tracei, w);
  }
  const bool stopped = S != 0;
  const int last_visited = stopped ? w : kend;
  if (use_f && kk <= last_visited && (skip || r1skip)) f = -1;
  if (stopped || kmax < 64) return 1;
  if (V) lt = __builtin_amdgcn_readlane(pf.h.tracei, 63 - __clzll((long long)V));  // every entry leaves its tracei
  return 2;
}

// Section D over the newest processed entries [0, kmax] in one wave step when the window holds entries
// with several active hits (s2_dloop_fast takes the all-single case): every hit the sequential walk
// would look at (entry by entry, each from its frontier) gets a lane, in walk order, when they number
// <= 64 and all sit in the ring.  The walk's sequential state reduces to:
//  - last_tr (range 0): an entry's hits are skipped while they carry the incoming last_tr, which then
//    becomes the first differing tracei, so each entry maps last_tr to its first tracei a, or (when
//    last_tr == a) to its first tracei b != a: a scalar pass over the entries (a few SALU each);
//  - the link: strict improvements over lanes in walk order are the records of a prefix max seeded
//    with the current score; the walk stops after the first entry whose last record has
//    consec >= ENOUGH_CONSECUTIVE, else the last record wins (the first lane holding the maximum);
//  - _mult's frontiers: per visited entry, the first hit past ranges 0-1, or -1.
// Fresh tracei values are drawn only for the winning range-2 link (values only meet in equality tests).
// Entries base .. base + 63 (pf loaded at base, lane = entry - base) from last_tr = lt; when their hits
// number more than 64 the leading entries whose hits fit are taken (a group) and the walk goes on from the
// next one (return 2, *next = its index, lt = last_tr there).
// Returns 0 (nothing done) when the window does not fit, else as s2_dloop_fast.
template <class SW>
__device__ __forceinline__ int s2_dloop_multi(SW& W, const S2Pref& pf, int np, int kmax, int q, uint32_t position,
                                              S2Best& b, bool range1, bool use_f, int& f, int& lt, int base = 0,
                                              int* next = nullptr) {
  const int kend = kmax - base < 63 ? kmax - base : 63;
  const int lane = W.lane;
  const int f0 = use_f ? f : 0;
  const bool inw0 = lane <= kend && base + lane < np && f0 != -1;
  // entries whose hits left the LDS ring (many active hits per entry) are gathered from global memory
  const bool inring = pf.n <= kS2Ring && pf.start >= W.pushed - kS2Ring;
  const int c0 = (inw0 && pf.n > 0) ? max(pf.n - f0, 0) : 0;
  const int incl0 = wave_incl_sum(c0, lane);
  // the group: the leading entries whose hits fit in the wave
  const uint64_t over = ballot(incl0 > 64);
  const int gend = over ? __ffsll((long long)over) - 1 : 64;  // entries [0, gend) of this window
  if (gend == 0 || (gend <= kend && !next)) return 0;
  const bool inw = inw0 && lane < gend;
  const bool valid = inw && pf.n > 0;
  const int c = valid ? c0 : 0;
  const int incl = wave_incl_sum(c, lane);
  const int total = __builtin_amdgcn_readlane(incl, 63);
  S2_TALLY(n_multi, 1);
  s2_uniform(b);
  if (b.consec >= kS2EnoughConsec) return 1;
  const int excl = incl - c;
  // one wave: its LDS operations run in order; the fence keeps the compiler from forwarding a lane's own
  // 0 to its load (other lanes' stores must be read back)
  s2_head[lane] = 0;
  if (c > 0) s2_head[excl] = lane + 1;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  const int hd = s2_head[lane];
  const uint64_t H = ballot(hd > 0);
  const bool act = lane < total;
  // this lane's hit: entry e (its first lane s), hit index k
  const uint64_t hb = H & ((2ull << lane) - 1ull);
  const int sl = hb ? 63 - __clzll((long long)hb) : 0;
  const int e = __shfl(hd, sl, 64) - 1;
  const int ee = e < 0 ? 0 : e;
  const int eq = __shfl(pf.q, ee, 64), est = __shfl(pf.start, ee, 64), ef = __shfl(f0, ee, 64),
            ec = __shfl(c, ee, 64), eoff = __shfl(pf.off, ee, 64), ering = __shfl((int)inring, ee, 64);
  const int k = ef + (lane - sl);
  S2HV v = {};
  if (ballot(act && !ering)) wave_sync();  // this wave's earlier global writes are complete
  if (act && ering) {
    const int r = (est + k) & (kS2Ring - 1);
    v.map = s2_ring.map[r];
    v.score = s2_ring.score[r];
    v.consec = s2_ring.consec[r];
    v.tracei = s2_ring.tracei[r];
    v.root = s2_ring.root[r];
    v.hit = s2_ring.hit[r];
  } else if (act) {
    v = s2_load_global(W.hits, W.maps, W.sc, W.alist, eoff, k);
  }
  const int eend = sl + ec;  // one past the entry's last lane
  const int a = __shfl(v.tracei, sl, 64);
  const uint64_t N = ballot(act && v.tracei != a);
  const uint64_t Nm = N & ~((1ull << sl) - 1ull);
  const int nx = Nm ? __ffsll((long long)Nm) - 1 : 64;
  const int nxt = nx < eend ? nx : eend;  // first lane of the entry whose tracei differs from a
  const int bt = __shfl(v.tracei, nx < eend ? nx : sl, 64);
  // range 0 across entries (scalar): eqm bit s set when the entry starting at lane s meets last_tr == a
  uint64_t eqm = 0, Hm = H;
  int last_tr = lt;
  while (Hm) {
    const int s0 = __ffsll((long long)Hm) - 1;
    Hm &= Hm - 1ull;
    const int as = __builtin_amdgcn_readlane(a, s0);
    if (last_tr == as) {
      eqm |= 1ull << s0;
      last_tr = __builtin_amdgcn_readlane(bt, s0);
    } else {
      last_tr = as;
    }
  }
  const bool skip0 = act && ((eqm >> sl) & 1ull) && lane < nxt;
  const int qd = q - eq;
  const bool r1 = act && !skip0 && range1 && v.map + W.maxintronlen + (uint32_t)qd <= position;
  int kind = 0, fs = INT_MIN;
  if (act && !skip0 && !r1) {
    if (v.map + (uint32_t)kS2EqualNotSplicing + (uint32_t)qd < position) {
      const int diff = (int)(position - v.map) - qd;
      kind = 2;
      fs = W.canon(v.score + (-qd / kS2K) - (W.splicingp ? (diff / kS2TenThousand + 1) : (diff + 1)), v.map, position,
                   qd, kS2FormMulti, false);
    } else if (v.map + (uint32_t)kS2K <= position) {
      kind = 4;
      fs = v.score + 1;
    }
  }
  const int im = wave_incl_max(fs, lane);
  int pm = __shfl_up(im, 1, 64);
  if (lane == 0) pm = INT_MIN;
  pm = max(pm, b.score);
  const bool rec = kind != 0 && fs > pm;
  int cons = 0;
  if (kind == 4) {
    const int g = (int)(position - v.map);
    const int diff = g > qd ? g - qd : qd - g;
    cons = (diff <= 0) ? v.consec + qd : 0;
  }
  const uint64_t R = ballot(rec);
  const uint64_t upto_end = eend >= 64 ? ~0ull : ((1ull << eend) - 1ull);
  const uint64_t after = ~((2ull << lane) - 1ull);
  const bool lastrec = rec && !(R & upto_end & after);
  const uint64_t S = ballot(lastrec && cons >= kS2EnoughConsec);
  int w = -1, stop_e = kend;
  if (S) {
    w = __ffsll((long long)S) - 1;
    stop_e = __builtin_amdgcn_readlane(e, w);
  } else if (R) {
    w = 63 - __clzll((long long)R);
  }
  S2_TALLY(n_cand, __popcll(R));
  if (w >= 0) {
    b.score = __builtin_amdgcn_readlane(fs, w);
    b.consec = __builtin_amdgcn_readlane(cons, w);
    b.root = __builtin_amdgcn_readlane(v.root, w);
    b.pp = __builtin_amdgcn_readlane(eq, w);
    b.ph = __builtin_amdgcn_readlane(v.hit, w);
    b.tracei = __builtin_amdgcn_readlane(kind, w) == 2 ? ++W.tracectr : __builtin_amdgcn_readlane(v.tracei, w);
  }
  if (use_f) {
    const uint64_t G = ballot(act && !skip0 && !r1);
    const uint64_t Gm = G & ~((1ull << (excl & 63)) - 1ull);
    const int g = Gm ? __ffsll((long long)Gm) - 1 : 64;
    if (inw && lane <= stop_e) f = (c > 0 && g < excl + c) ? f0 + (g - excl) : -1;
  }
  if (S) return 1;
  lt = last_tr;  // (also at the window's end: a caller whose window stops short of the walk's goes on)
  if (gend <= kend) {  // the hits of the later entries did not fit this group
    *next = base + gend;
    return 2;
  }
  if (kmax - base < 64) return 1;
  if (next) *next = base + 64;
  return 2;
}

// score_querypos_lookback_one (stage2.c:1073); returns the link
template <class SW>
__device__ __forceinline__ S2Best s2_one(SW& W, int q, uint32_t position, int np, const S2E& last) {
  S2Best b = {kS2K, (int)position, -1, -1, 0, 0};
  int nlookback = kS2Nsufflookback, lookback = kS2Sufflookback;
  S2_SUB_DECL();
  if (np > 0) {
    S2_SUB_T0();
    int k = last.n > 0 ? 0 : -1;
    S2HV u;
    if (s2_adj(W, last, k, q - last.q, position, u)) {
      b.consec = u.consec + (q - last.q);
      b.root = u.root;
      b.score = u.score + (q - last.q);
      b.pp = last.q;
      b.ph = u.hit;
      b.tracei = u.tracei;
      nlookback = 1;
      lookback = kS2Sufflookback / 2;
    }
    S2_SUB(0);
  }
  s2_uniform(b);
  bool donep = false;
  int last_tr = -1;
  if (np > 0 && b.consec < kS2EnoughConsec) {
    S2_SUB_T0();
    S2Pref pf;
    pf.load(W, np);
    // the entry that ends the walk (donep): the first beyond nlookback more than lookback + 8 back
    const uint64_t dm = ballot(W.lane < np && W.lane > nlookback && (q - pf.q) - kS2K > lookback);
    const int kmax = dm ? __ffsll((long long)dm) - 1 : (np <= 64 ? np - 1 : 64);
    int fdummy = 0, lt = -1, from = 0;
    S2_SUB(1);
    int st;
    S2_SUB_T0();
    st = s2_dloop_fast(W, pf, np, kmax, q, position, b, W.splicingp != 0, false, fdummy, lt);
    S2_SUB(2);
    S2_SUB_T0();
    if (st == 2) from = 64;
    if (!st) {  // entries with several hits: groups of entries whose hits fit the wave
      // (when the walk goes past the window, donep decides beyond it: the groups stop at entry 63 and a
      // window walked to its end without a stop goes on from entry 64)
      const int kg = kmax >= 64 ? 63 : kmax;
      S2Pref pg = pf;  // (a value, not a reference chosen at run time: that kept both windows in scratch)
      for (;;) {
        int nb = from;
        st = s2_dloop_multi(W, pg, np, kg, q, position, b, W.splicingp != 0, false, fdummy, lt, from, &nb);
        if (st != 2) break;
        from = nb;
        pg.load(W, np, from);
      }
      if (st == 1 && kmax >= 64 && b.consec < kS2EnoughConsec) {  // (a stop leaves consec >= ENOUGH)
        st = 2;
        from = 64;
      }
    }
    S2_SUB(3);
    S2_SUB_T0();
    if (st == 1) np = 0;  // done
    if (st != 1) last_tr = lt;
    S2EntryCache ec;
    for (int kk = from; kk < np && b.consec < kS2EnoughConsec && !donep; kk++) {
      const int eq = kk < kS2Pref ? __builtin_amdgcn_readlane(pf.q, kk) : ec.get(W, np, kk).q;
      if (kk > nlookback && (q - eq) - kS2K > lookback) donep = true;
      int qd;
      (void)s2_entry_eval(W, pf, ec, np, kk, 0, q, position, last_tr, b, W.splicingp != 0, &qd);
    }
    S2_SUB(4);
  }
  s2_uniform(b);
  if (b.pp < 0) {  // localp: indexsize; else the search's score, 0 (stage2.c:1445-1451)
    b.tracei = ++W.tracectr;
    if constexpr (SW::kLocalp) b.score = kS2K;
  }
  return b;
}

template <class SW>
__device__ __forceinline__ void s2_store_link(SW& W, int offq, int hit, const S2Best& b) {
  if (W.lane == 0) {
    W.hits[offq + hit] = S2Hit{b.consec, b.root, b.tracei, b.ph};  // (ph: -1 with pp)
    W.sc[offq + hit] = b.score;
  }
}

// score_querypos_lookback_mult (stage2.c:1470) over hits [low, high) of q; links to global
template <class SW>
__device__ __forceinline__ void s2_mult(SW& W, int q, int offq, int low, int high, int np, const S2E& last) {
  int* fr = s2_fr;
  const int nhits = high - low;
  if constexpr (SW::kCanon) W.in_mult = 1;
  if (np == 0) {
    for (int i = W.lane; i < nhits; i += 64) {
      W.hits[offq + low + i] = S2Hit{kS2K, (int)W.maps[offq + low + i], W.tracectr + 1 + i, -1};
      if constexpr (SW::kLocalp) W.sc[offq + low + i] = kS2K;
      else W.sc[offq + low + i] = 0;  // (:1555; its fwd_tracei stays unset: the restart below gives it -1)
    }
    W.tracectr += nhits;
    wave_sync();
    return;
  }
  const int adq = q - last.q;
  int maxadj = 0, maxnon = 0, nfr = 0;
  S2EntryCache ec;
  for (int n = 0; n < np && n < 128; n++) {
    const S2E e = ec.get(W, np, n);
    const int qd = q - e.q;
    if (n > kS2Nsufflookback && n > 1 && qd - kS2K > kS2Sufflookback) break;  // later entries only shrink
    if (n <= 1 || qd - kS2K <= kS2Sufflookback / 2) maxadj = n;
    if (n <= kS2Nsufflookback || qd - kS2K <= kS2Sufflookback) maxnon = n;
    if (W.lane == 0) fr[n] = e.n > 0 ? 0 : -1;
    nfr = n + 1;
  }
  wave_sync();
  int overall = 0, adjf = last.n > 0 ? 0 : -1;
  for (int i = 0; i < nhits; i++) {
    const uint32_t position = W.maps[offq + low + i];
    S2HV u;
    if (s2_adj(W, last, adjf, adq, position, u) && u.consec + adq > overall) overall = u.consec + adq;
  }
  adjf = last.n > 0 ? 0 : -1;
  for (int i = 0; i < nhits; i++) {
    const uint32_t position = W.maps[offq + low + i];
    S2Best b;
    int maxseen;
    S2HV u;
    if (s2_adj(W, last, adjf, adq, position, u)) {
      b = {u.consec + adq, u.root, last.q, u.hit, u.score + adq, u.tracei};
      maxseen = maxadj;
    } else {
      b = {kS2K, (int)position, -1, -1, 0, -1};
      maxseen = maxnon;
    }
    if (overall < kS2GreedyConsec) {
      int last_tr = -1;
      for (int kk = 0; kk < np && b.consec < kS2EnoughConsec && kk <= maxseen && kk < nfr; kk++) {
        const int f = s2_u(s2_fr[kk]);
        if (f != -1) {
          const S2E e = ec.get(W, np, kk);
          const int nf = s2_eval(W, e, f, q, position, last_tr, b, true);
          wave_sync();
          if (W.lane == 0) fr[kk] = nf;
          wave_sync();
        }
      }
    }
    if (b.pp < 0) {
      b.tracei = ++W.tracectr;
      if constexpr (SW::kLocalp) b.score = kS2K;
    }
    s2_store_link(W, offq, low + i, b);
  }
  if constexpr (SW::kCanon) W.in_mult = 0;
  wave_sync();
}

// the members of a run (s2_sweep): lane = query position cb + lane, members Mm; links, active lists and
// ring slots (its own function: the sweep's register budget is full)
struct S2Run {
  int score, consec, tracei, root, hit, q, pushed, np;
};
// hit: the member's index at its position (off: the position's first hit), prev: the previous member's
// index within the call (the link of every member but the first, which links to L.hit)
__device__ __forceinline__ void s2_run_write(S2Hit* hits, int* sc, int* alist, int lane, int off, int hit,
                                             int prev, uint32_t map, int qq, S2Run L, uint64_t Mm) {
  if (!((Mm >> lane) & 1ull)) return;
  const uint64_t below = Mm & ((1ull << lane) - 1ull);
  const int r = __popcll(below);
  const int dq = qq - L.q;
  hits[off + hit] = S2Hit{L.consec + dq, L.root, L.tracei, below ? prev : L.hit};
  sc[off + hit] = L.score + dq;
  alist[off] = hit;
  const int sl = (L.pushed + r) & (kS2Ring - 1);
  s2_ring.map[sl] = map;
  s2_ring.score[sl] = L.score + dq;
  s2_ring.consec[sl] = L.consec + dq;
  s2_ring.tracei[sl] = L.tracei;
  s2_ring.root[sl] = L.root;
  s2_ring.hit[sl] = off + hit;
  const int ms = (L.np + r) & (kS2Meta - 1);
  s2_ring.eq[ms] = qq;
  s2_ring.en[ms] = 1;
  s2_ring.eoff[ms] = off;
  s2_ring.estart[ms] = L.pushed + r;
}

// the sweep (stage2.c:3746-4080)
template <class SW>
__device__ __forceinline__ void s2_sweep(SW& W, const int32_t* npq, int nq, const int* fp, const uint32_t* rmapa,
                                         int qstart, int qend) {
  const int lane = W.lane;
  auto npos = [&](int q) { return q < nq ? npq[q] : 0; };
  int q = 0, np = 0;
  for (int i = lane; i < qstart; i += 64) W.actn[i] = 0;
  q = qstart;
  while (q <= qend && npos(q) <= 0) {
    if (lane == 0) W.actn[q] = 0;
    q++;
  }
  // The first position with hits keeps every hit in the layout, its active range [low0, high0) beside it;
  // any other position's laid-out hits are its active range (s2a_kernel)
  const int q0 = q;
  int low0 = 0, high0 = 0;
  if (q <= qend) {  // the first position with hits: every hit starts a path
    const int n = npos(q), offq = W.off[q];
    low0 = s2_u(fp[0]);
    high0 = s2_u(fp[1]);
    for (int i = lane; i < n; i += 64) {
      // (root 0: the CALLOC'ed value the reference leaves, stage2.c:3760-3770)
      W.hits[offq + i] = S2Hit{kS2K, 0, -1, -1};
      W.sc[offq + i] = kS2K;
    }
  }
  wave_sync();
  int grand_score = 0, grand_q = -1, grand_hit = -1, nskipped = 0, min_hits = 1000000, specific_q = -1,
      specific_low = 0, specific_high = 0;
  uint32_t grand_map = 0;
  S2E last = {0, 0, 0, 0, false};
  // per-position metadata for the chunk [cb, cb + 64): npositions, off, and the hits inside [minactive,
  // maxactive]: [m_low, m_high) = [0, off[q + 1] - off[q]) but at q0, m_rmap the first of them (s2a_kernel)
  int cb = -1, m_n = 0, m_off = 0, m_low = 0, m_high = 0;
  uint32_t m_rmap = 0;
#ifdef GMAPDP_OI_TIMING
  unsigned long long t_one = 0, t_mult = 0, t_tail = 0, t_meta = 0, t0c = 0;
#define S2_T0() t0c = wall_clock64()
#define S2_TACC(acc) (acc += wall_clock64() - t0c, t0c = wall_clock64())
#else
#define S2_T0() (void)0
#define S2_TACC(acc) (void)0
#endif
  while (q <= qend) {
    S2_T0();
    W.tracectr = s2_u(W.tracectr);
    W.pushed = s2_u(W.pushed);
    if ((q & ~63) != cb) {
      cb = q & ~63;
      const int qq = cb + lane;
      const bool in = qq <= qend;
      m_n = qq < nq ? npq[qq] : 0;
      m_off = qq <= qend + 1 ? W.off[qq] : 0;
      const int o1 = in ? W.off[qq + 1] : 0;  // (qend < querylength: off[qend + 1] exists)
      m_low = qq == q0 ? low0 : 0;
      m_high = qq == q0 ? high0 : o1 - m_off;
      m_rmap = in ? rmapa[qq] : 0u;
    }
    const int j = q - cb;
    // A run on the last processed entry's diagonal.  When that entry has one active hit whose consecutive
    // count reaches ENOUGH_CONSECUTIVE by the next position on its diagonal, every following position
    // whose only hit in the active range sits on that diagonal takes section A's link (stage2.c:1126-1168)
    // and skips section D (:1191): score and consec grow by the query distance, root and tracei carry
    // over, the link points at the previous such position, the hit stays active (score > 0), and the
    // grand lookback (:3983) does not apply (the link has a predecessor).  Positions without hits in
    // between change nothing (they are not processed entries).  So the chunk's run of such positions is
    // written lane-parallel in one step: links, active lists, the ring, the grand best.
    if (last.n == 1 && last.inring && nskipped <= kS2MaxSkipped) {
      const int ls = last.start & (kS2Ring - 1);
      const uint32_t lmap = s2_u(s2_ring.map[ls]);
      const int lcons = s2_u(s2_ring.consec[ls]);
      const uint32_t dg = lmap - (uint32_t)last.q;
      const int qq = cb + lane;
      const bool one = qq <= qend && m_high - m_low == 1 && m_rmap - (uint32_t)qq == dg;
      const uint64_t from_j = ~0ull << j;
      const uint64_t notE = ~ballot(qq <= qend && (m_n <= 0 || one)) & from_j;
      const int stop = notE ? __ffsll((long long)notE) - 1 : 64;
      const uint64_t inrun = stop >= 64 ? from_j : (from_j & ((1ull << stop) - 1ull));
      const uint64_t Mm = ballot(one) & inrun;
      if (Mm && lcons + (cb + __ffsll((long long)Mm) - 1 - last.q) >= kS2EnoughConsec) {
        const int lscore = s2_u(s2_ring.score[ls]), ltr = s2_u(s2_ring.tracei[ls]), lroot = s2_u(s2_ring.root[ls]),
                  lhit = s2_u(s2_ring.hit[ls]);
        const uint64_t mb = Mm & ((1ull << lane) - 1ull);
        const int prev = __shfl(m_off + m_low, mb ? 63 - __clzll((long long)mb) : 0, 64);
        s2_run_write(W.hits, W.sc, W.alist, lane, m_off, m_low, prev, m_rmap, qq,
                     {lscore, lcons, ltr, lroot, lhit, last.q, W.pushed, np}, Mm);
        if ((inrun >> lane) & 1ull) W.actn[qq] = (int)((Mm >> lane) & 1ull);
        const int cnt = __popcll(Mm);
        S2_TALLY(n_runs, 1);
        S2_TALLY(n_runpos, cnt);
        const int ll = 63 - __clzll((long long)Mm);
        const int lq = cb + ll;
        const int lsc = lscore + (lq - last.q);
        if (lsc >= grand_score) {  // consec >= ENOUGH_CONSECUTIVE > EXON_DEFN
          grand_score = lsc;
          grand_q = lq;
          grand_hit = __builtin_amdgcn_readlane(m_off + m_low, ll);
          grand_map = (uint32_t)__builtin_amdgcn_readlane((int)m_rmap, ll);
        }
        const int loff = __builtin_amdgcn_readlane(m_off, ll);
        W.pushed += cnt;
        np += cnt;
        last = s2_mkentry(W, lq, 1, loff, W.pushed - 1);
        nskipped = 0;
        min_hits = 1000000;
        specific_q = -1;
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __builtin_amdgcn_wave_barrier();
        S2_TACC(t_one);
        q = cb + stop;
        continue;
      }
    }
    const int n = __builtin_amdgcn_readlane(m_n, j);
    const int offq = __builtin_amdgcn_readlane(m_off, j);
    int low = __builtin_amdgcn_readlane(m_low, j), high = __builtin_amdgcn_readlane(m_high, j);
    if constexpr (SW::kSkipRepetitive) {
      if (high - low >= kS2MaxNactive && nskipped <= kS2MaxSkipped) {
        if (lane == 0) W.actn[q] = 0;
        nskipped++;
        if (high - low < min_hits) {
          min_hits = high - low;
          specific_q = q;
          specific_low = low;
          specific_high = high;
        }
        q++;
        continue;
      }
    }
    int next_q, qoff = offq;
    if (nskipped > kS2MaxSkipped) {
      next_q = q;
      q = specific_q;
      low = specific_low;
      high = specific_high;
      qoff = W.off[q];
    } else {
      next_q = q + 1;
    }
    S2_TACC(t_meta);
    int nact = 0;
    if (high - low == 1) {
      // one hit in the active range (the common case): everything stays in registers and LDS
      const uint32_t position = (q == cb + j) ? (uint32_t)__builtin_amdgcn_readlane((int)m_rmap, j)
                                              : W.maps[qoff + low];
      S2Best b = s2_one(W, q, position, np, last);
      int best_score = b.score > 0 ? b.score : 0;
      const bool have_best = b.score > 0;
      if constexpr (!SW::kMiddlep) {
        // a new start (stage2.c:3955-3980; best_fwd_hit stays -1: no grand lookback, no new grand best).  It
        // takes every hit of the position; these calls' bounds (Diag_max_bounds) leave none outside [low, high)
        if (!have_best) b = {kS2K, b.root, -1, -1, kS2K, -1};
      }
      nskipped = 0;
      min_hits = 1000000;
      specific_q = -1;
      if (W.splicingp && have_best && b.ph < 0 && grand_q >= 0 && q >= grand_q + kS2K) {
        if ((best_score = grand_score - (q - grand_q)) > 0) {
          if (!(position > grand_map + W.maxintronlen) && position >= grand_map + (uint32_t)kS2K) {
            b.consec = kS2K;
            b.pp = grand_q;
            b.ph = grand_hit;
            b.tracei = ++W.tracectr;
            b.score = best_score;
          }
        }
      }
      if (have_best && best_score >= grand_score && b.consec > kS2ExonDefn) {
        grand_score = best_score;
        grand_q = q;
        grand_hit = qoff + low;
        grand_map = position;
      }
      s2_store_link(W, qoff, low, b);
      const int threshold = max(b.score - kS2ScoreRestrict, 0);
      if (b.score > threshold) {
        nact = 1;
        if (lane == 0) {
          W.alist[qoff] = low;
          const int sl = W.pushed & (kS2Ring - 1);
          s2_ring.map[sl] = position;
          s2_ring.score[sl] = b.score;
          s2_ring.consec[sl] = b.consec;
          s2_ring.tracei[sl] = b.tracei;
          s2_ring.root[sl] = b.root;
          s2_ring.hit[sl] = qoff + low;
        }
      }
    } else if (high - low > 1 && high - low <= 64) {
      // several hits (<= 64): lane i holds hit low + i and its link
      const int nh = high - low;
      S2_SUB_DECL();
      S2_SUB_T0();
      const uint32_t cm = lane < nh ? W.maps[qoff + low + lane] : 0u;
      S2Best mb = {0, 0, -1, -1, 0, 0};
      if (np == 0) {
        if (lane < nh) mb = {kS2K, (int)cm, -1, -1, SW::kLocalp ? kS2K : 0, W.tracectr + 1 + lane};
        W.tracectr += nh;
      } else {
        const int adq = q - last.q;
        S2Pref pf;
        pf.load(W, np);
        S2EntryCache ec;
        // the entries any hit of q may look back to (stage2.c:1470's maxadj / maxnon bounds) and their
        // frontiers, 64 entries per wave step: qd grows with n, so each bound is the last lane of a ballot
        int maxadj = 0, maxnon = 0, nfr = 0;
        for (int base = 0; base < np && base < 128; base += 64) {
          const int n = base + lane;
          const bool in = n < np && n < 128;
          int eq = pf.q, en = pf.n;
          if (base) {
            const int k = (np - 1 - n) & (kS2Meta - 1);
            eq = in ? s2_ring.eq[k] : 0;
            en = in ? s2_ring.en[k] : 0;
          }
          const int qd = q - eq;
          const uint64_t B = ballot(in && n > kS2Nsufflookback && n > 1 && qd - kS2K > kS2Sufflookback);
          const int lim = B ? __ffsll((long long)B) - 1 : 64;  // later entries only shrink
          const bool v = in && lane < lim;
          const uint64_t A = ballot(v && (n <= 1 || qd - kS2K <= kS2Sufflookback / 2));
          const uint64_t M = ballot(v && (n <= kS2Nsufflookback || qd - kS2K <= kS2Sufflookback));
          if (A) maxadj = base + 63 - __clzll((long long)A);
          if (M) maxnon = base + 63 - __clzll((long long)M);
          if (v) s2_fr[n] = en > 0 ? 0 : -1;
          const uint64_t Vm = ballot(v);
          if (Vm) nfr = base + 64 - __clzll((long long)Vm);
          if (B || !(Vm >> 63)) break;
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        // Section A for every hit at once when the last entry's active hits are in the ring: both lists
        // ascend, so hit i's adjacent hit is the first active one with map + adq >= its position (what
        // s2_adj's frontier walk finds), by a binary search per lane
        const bool par_adj = last.n > 0 && last.inring;
        bool a_found = false;
        S2HV a_u = {};
        int overall = 0, adjf = last.n > 0 ? 0 : -1;
        if (par_adj) {
          if (lane < nh) {
            int lo = 0, hi = last.n;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (s2_ring.map[(last.start + mid) & (kS2Ring - 1)] + (uint32_t)adq >= cm) hi = mid;
              else lo = mid + 1;
            }
            if (lo < last.n) {
              const int sl = (last.start + lo) & (kS2Ring - 1);
              if (s2_ring.map[sl] + (uint32_t)adq == cm) {
                a_found = true;
                a_u.map = cm;
                a_u.score = s2_ring.score[sl];
                a_u.consec = s2_ring.consec[sl];
                a_u.tracei = s2_ring.tracei[sl];
                a_u.root = s2_ring.root[sl];
                a_u.hit = s2_ring.hit[sl];
              }
            }
          }
          overall = max(wave_max_i(a_found ? a_u.consec + adq : 0), 0);
        } else {
          for (int i = 0; i < nh; i++) {
            const uint32_t position = (uint32_t)__builtin_amdgcn_readlane((int)cm, i);
            S2HV u;
            if (s2_adj(W, last, adjf, adq, position, u) && u.consec + adq > overall) overall = u.consec + adq;
          }
        }
        const uint64_t a_mask = ballot(a_found);
        adjf = last.n > 0 ? 0 : -1;
        S2_SUB(6);
        for (int i = 0; i < nh; i++) {
          const uint32_t position = (uint32_t)__builtin_amdgcn_readlane((int)cm, i);
          S2Best b;
          int maxseen;
          S2HV u;
          bool adjacent;
          if (par_adj) {
            adjacent = (a_mask >> i) & 1ull;
            if (adjacent) u = s2_bcast(a_u, i);
          } else {
            adjacent = s2_adj(W, last, adjf, adq, position, u);
          }
          if (adjacent) {
            b = {u.consec + adq, u.root, last.q, u.hit, u.score + adq, u.tracei};
            maxseen = maxadj;
          } else {
            b = {kS2K, (int)position, -1, -1, 0, -1};
            maxseen = maxnon;
          }
          s2_uniform(b);
          int st = 0, lt = -1, from = 0;
          S2_SUB_T0();
          if (overall < kS2GreedyConsec) {
            const int kmax = min(min(maxseen, nfr - 1), np - 1);
            const int kend = min(kmax, 63);
            int f = lane <= kend ? s2_fr[lane] : -1;
            st = s2_dloop_fast(W, pf, np, kmax, q, position, b, true, true, f, lt);
            if (st && lane <= kend) s2_fr[lane] = f;
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            if (st == 2) from = 64;
            if (!st) {  // groups of entries whose hits fit the wave, from entry 0
              lt = -1;
              st = 2;
            }
            S2Pref pg = pf;  // (a value: a reference chosen at run time kept both windows in scratch)
            while (st == 2 && from <= kmax) {
              if (from) pg.load(W, np, from);
              const S2Pref& pw = pg;
              const int ke = min(kmax - from, 63);
              int fg = lane <= ke ? s2_fr[from + lane] : -1;
              int nb = from;
              const int r = s2_dloop_multi(W, pw, np, kmax, q, position, b, true, true, fg, lt, from, &nb);
              if (r && lane <= ke) s2_fr[from + lane] = fg;
              __atomic_signal_fence(__ATOMIC_SEQ_CST);
              st = r;
              if (r == 2) from = nb;
            }
            if (st == 2) st = 1;  // every entry up to kmax walked
          }
          S2_SUB(7);
          S2_SUB_T0();
          if (overall < kS2GreedyConsec && st != 1) {
            int last_tr = lt;
            for (int kk = from; kk < np && b.consec < kS2EnoughConsec && kk <= maxseen && kk < nfr;
                 kk++) {
              const int f = s2_u(s2_fr[kk]);
              if (f != -1) {
                int qd;
                const int nf = s2_entry_eval(W, pf, ec, np, kk, f, q, position, last_tr, b, true, &qd);
                if (lane == 0) s2_fr[kk] = nf;
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
              }
            }
          }
          S2_SUB(5);
          s2_uniform(b);
          if (b.pp < 0) {
            b.tracei = ++W.tracectr;
            if constexpr (SW::kLocalp) b.score = kS2K;
          }
          if (lane == i) mb = b;
        }
      }
      // best of the position: the first hit with the maximal score (> 0)
      const int sc = lane < nh ? mb.score : INT_MIN;
      const int smax = wave_max_i(sc);
      int best_score = 0, best_hit = -1, bl = 0;
      if (smax > 0) {
        bl = __ffsll((long long)ballot(lane < nh && sc == smax)) - 1;
        best_score = smax;
        best_hit = low + bl;
      }
      if constexpr (!SW::kMiddlep) {  // a new start for every hit (:3955-3980); root stays the hit's own position
        if (best_hit < 0 && lane < nh) mb = {kS2K, (int)cm, -1, -1, kS2K, -1};
      }
      nskipped = 0;
      min_hits = 1000000;
      specific_q = -1;
      if (W.splicingp && best_hit >= 0 && __builtin_amdgcn_readlane(mb.ph, bl) < 0 && grand_q >= 0 &&
          q >= grand_q + kS2K) {
        if ((best_score = grand_score - (q - grand_q)) > 0) {
          if (lane < nh && !(cm > grand_map + W.maxintronlen) && cm >= grand_map + (uint32_t)kS2K) {
            mb.consec = kS2K;
            mb.pp = grand_q;
            mb.ph = grand_hit;
            mb.tracei = W.tracectr + 1 + lane;  // fresh per relinked hit
            mb.score = best_score;
          }
          W.tracectr += nh;
        }
      }
      if (best_hit >= 0 && best_score >= grand_score && __builtin_amdgcn_readlane(mb.consec, bl) > kS2ExonDefn) {
        grand_score = best_score;
        grand_q = q;
        grand_hit = qoff + best_hit;
        grand_map = (uint32_t)__builtin_amdgcn_readlane((int)cm, bl);
      }
      if (lane < nh) {
        W.hits[qoff + low + lane] = S2Hit{mb.consec, mb.root, mb.tracei, mb.ph};
        W.sc[qoff + low + lane] = mb.score;
      }
      // revise_active_lookback + the entry's active hits into the ring
      const int threshold = max(wave_max_i(lane < nh ? mb.score : INT_MIN) - kS2ScoreRestrict, 0);
      const bool a = lane < nh && mb.score > threshold;
      const uint64_t am = ballot(a);
      if (a) {
        const int r = lanes_below(am, lane);
        W.alist[qoff + r] = low + lane;
        const int sl = (W.pushed + r) & (kS2Ring - 1);
        s2_ring.map[sl] = cm;
        s2_ring.score[sl] = mb.score;
        s2_ring.consec[sl] = mb.consec;
        s2_ring.tracei[sl] = mb.tracei;
        s2_ring.root[sl] = mb.root;
        s2_ring.hit[sl] = qoff + low + lane;
      }
      nact = __popcll(am);
    } else {
      int best_score = 0, best_hit = -1, best_fhit = 0, best_consec = 0;
      if (high - low > 1) {
        S2_SUB_DECL();
        S2_SUB_T0();
        s2_mult(W, q, qoff, low, high, np, last);
        S2_SUB(5);
        int bs = 0, bh = -1;
        for (int c0 = low; c0 < high; c0 += 64) {
          const int i = c0 + lane;
          const int sc = i < high ? W.sc[qoff + i] : INT_MIN;
          const int m = wave_max_i(sc);
          if (m > bs) {
            bs = m;
            bh = c0 + __ffsll((long long)ballot(i < high && sc == m)) - 1;
          }
        }
        best_score = bs;
        best_hit = bh;
        if constexpr (!SW::kMiddlep) {  // a new start for every hit (:3955-3980)
          if (bh < 0) {
            for (int i = low + lane; i < high; i += 64) {
              W.hits[qoff + i] = S2Hit{kS2K, (int)W.maps[qoff + i], -1, -1};
              W.sc[qoff + i] = kS2K;
            }
            wave_sync();
          }
        }
        if (bh >= 0) {
          best_fhit = W.hits[qoff + bh].pred;
          best_consec = W.hits[qoff + bh].consec;
        }
        nskipped = 0;
        min_hits = 1000000;
        specific_q = -1;
        if (W.splicingp && best_hit >= 0 && best_fhit < 0 && grand_q >= 0 && q >= grand_q + kS2K) {
          if ((best_score = grand_score - (q - grand_q)) > 0) {  // fwd_scores[grand] is grand_score
            for (int i = low + lane; i < high; i += 64) {
              S2Hit& x = W.hits[qoff + i];
              const uint32_t xmap = W.maps[qoff + i];
              if (xmap > grand_map + W.maxintronlen) continue;
              if (xmap >= grand_map + (uint32_t)kS2K) {
                x.consec = kS2K;
                x.pred = grand_hit;
                x.tracei = W.tracectr + 1 + (i - low);  // fresh per relinked hit
                W.sc[qoff + i] = best_score;
              }
            }
            W.tracectr += high - low;
            wave_sync();
            best_consec = W.hits[qoff + best_hit].consec;
          }
        }
        if (best_hit >= 0 && best_score >= grand_score && best_consec > kS2ExonDefn) {
          grand_score = best_score;
          grand_q = q;
          grand_hit = qoff + best_hit;
          grand_map = W.maps[qoff + best_hit];
        }
        // revise_active_lookback + the entry's active hits into the ring
        int best = INT_MIN;
        for (int c0 = low; c0 < high; c0 += 64) {
          const int i = c0 + lane;
          best = max(best, i < high ? W.sc[qoff + i] : INT_MIN);
        }
        const int threshold = max(wave_max_i(best) - kS2ScoreRestrict, 0);
        for (int c0 = low; c0 < high; c0 += 64) {
          const int i = c0 + lane;
          S2Hit x = {};
          uint32_t xmap = 0;
          int xscore = 0;
          bool a = false;
          if (i < high) {
            x = W.hits[qoff + i];
            xmap = W.maps[qoff + i];
            xscore = W.sc[qoff + i];
            a = xscore > threshold;
          }
          const uint64_t m = ballot(a);
          if (a) {
            const int r = nact + lanes_below(m, lane);
            W.alist[qoff + r] = i;
            if (high - low <= kS2Ring) {
              const int sl = (W.pushed + r) & (kS2Ring - 1);
              s2_ring.map[sl] = xmap;
              s2_ring.score[sl] = xscore;
              s2_ring.consec[sl] = x.consec;
              s2_ring.tracei[sl] = x.tracei;
              s2_ring.root[sl] = x.root;
              s2_ring.hit[sl] = qoff + i;
            }
          }
          nact += __popcll(m);
        }
      }
    }
    if (high - low == 1) S2_TACC(t_one); else S2_TACC(t_mult);
    if (high - low == 1) S2_TALLY(n_onepos, 1); else if (high - low > 1) S2_TALLY(n_multpos, 1);
    if (lane == 0) W.actn[q] = nact;
    if ((q == cb + j ? n : npos(q)) > 0) {  // the prefetched count unless the MAX_SKIPPED jump moved q
      const bool ringed = high - low <= kS2Ring;
      const int start = ringed ? W.pushed : W.pushed - 2 * kS2Ring;  // never in the ring
      if (lane == 0) {
        const int s = np & (kS2Meta - 1);
        s2_ring.eq[s] = q;
        s2_ring.en[s] = nact;
        s2_ring.eoff[s] = qoff;
        s2_ring.estart[s] = start;
      }
      if (ringed) W.pushed += nact;
      np++;
      last = s2_mkentry(W, q, nact, qoff, start);
    }
    // one wave: its LDS operations execute in order, so the ring writes above are visible to the next
    // position's reads; only the compiler must not move memory operations across this point.  Global
    // data written here is read back only after a full wait (wave_sync) on the slow paths.
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_wave_barrier();
    S2_TACC(t_tail);
    q = next_q;
  }
  S2_COUNT(8, t_meta);
  S2_COUNT(9, t_one);
  S2_COUNT(10, t_mult);
  S2_COUNT(11, t_tail);
#ifdef GMAPDP_OI_TIMING
  S2_COUNT(13, W.n_cand);
  S2_COUNT(14, W.n_fast);
  S2_COUNT(15, W.n_slow);
  if (threadIdx.x == 0) {
    atomicAdd(&g_s2_marks[1][15], W.n_multi);
    atomicAdd(&g_s2_marks[1][8], W.n_runs);
    atomicAdd(&g_s2_marks[1][9], W.n_runpos);
    atomicAdd(&g_s2_marks[1][10], W.n_onepos);
    atomicAdd(&g_s2_marks[1][11], W.n_multpos);
    for (int k = 0; k < 8; k++) {
      atomicAdd(&g_s2_sub[0][k], W.sub[k]);
      atomicAdd(&g_s2_sub[1][k], W.subn[k]);
    }
  }
#endif
}

__device__ __forceinline__ char s2_genomic_nt(const uint32_t* __restrict__ blocks, uint64_t nwords, uint32_t chrpos,
                                              uint64_t chroffset, uint64_t chrhigh, bool plusp) {
  // get_genomic_nt (stage2.c:4124): no chromosome-bound check
  const char c = decode_nt(blocks, nwords, plusp ? chroffset + chrpos : chrhigh - chrpos);
  return plusp ? c : compl_nt(c);
}

// traceback_one (stage2.c:4140): drop the 3'-end links with fewer than MIN_TERMINAL_NCONSECUTIVE
// consecutive matches, then visit the path's hits 3' end first (Pairpool_push drops chrpos >= 2^31)
// The query position of hit h (its index within the call): the last q with off[q] <= h.  off[0 .. ql]
// ascends from 0 to the hit count, and a position without hits shares its successor's offset, so that q
// is the one position whose hits include h.  One lane: a binary search.
__device__ __forceinline__ int s2_hit_pos(const int* __restrict__ off, int ql, int h) {
  int lo = 0, hi = ql;  // off[lo] <= h < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= h) lo = mid;
    else hi = mid;
  }
  return lo;
}
// The same for a wave-uniform h by the whole wave: 64 probes per round trip (two for a 2-kb query)
__device__ __forceinline__ int s2_hit_pos_wave(const int* __restrict__ off, int ql, int h, int lane) {
  int lo = 0, hi = ql;  // off[lo] <= h < off[hi]
  while (hi - lo > 1) {
    const int step = (hi - lo + 63) >> 6;
    const int p = lo + lane * step;  // lane 0 probes lo itself: true
    const uint64_t m = ballot(p < hi && off[p] <= h);  // a prefix of the lanes
    lo += (63 - __clzll((long long)m)) * step;
    hi = min(hi, lo + step);
  }
  return lo;
}

template <class F>
__device__ void s2_walk(const S2Hit* hits, const uint32_t* maps, const int* off, int ql, int gi, F visit) {
  while (gi >= 0 && hits[gi].consec < kS2MinTerminal) gi = hits[gi].pred;
  if (gi < 0) return;
  int q = s2_hit_pos(off, ql, gi);
  while (gi >= 0) {
    if ((int)maps[gi] >= 0) visit(gi, q);
    gi = hits[gi].pred;
    if (gi >= 0)  // a link goes to an earlier position: step down to the one holding gi
      while (q > 0 && off[--q] > gi) {
      }
  }
}

// convert_to_nucleotides (stage2.c:5334) for path entry e (3' end first): fill pairs between it and
// the entry before, and whether a gap holder precedes them
__device__ __forceinline__ void s2_entry_v(int e, int qpos, int gpos, int lq, int lg, int& fill, int& gap) {
  gap = 0;
  if (e == 0) {
    fill = kS2K - 1;
    return;
  }
  const int qj = lq - 1 - qpos, gj = lg - 1 - gpos;
  if (qj == 0 && gj == 0) {
    fill = 0;
    return;
  }
  if (qpos + kS2K - 1 >= lq || gpos + kS2K - 1 >= lg)
    fill = (lq - qpos < lg - gpos) ? lq - qpos - 1 : lg - gpos - 1;
  else
    fill = kS2K - 1;
  gap = ((gj - fill) > 0 || (qj - fill) > 0) ? 1 : 0;
}

// Launch order of the chaining kernels: blockIdx -> problem, the calls with the most seeding hits first.
// A wave's sweep time grows with its hits (tools/oi_timing.py s2: correlation 0.89, 6.6 ms median and
// 17.7 ms slowest per wave on the bench's reads), and the grid is ~1.4 waves of residency deep, so a
// heavy call dispatched late sets the kernel's end; longest-first leaves the light ones for the tail.
// The order sits after the four counters in the counters buffer (s2_order_kernel writes it).
__device__ __forceinline__ int s2_problem(const unsigned long long* counters) {
  return reinterpret_cast<const int*>(counters + 4)[blockIdx.x];
}

constexpr int kS2OrderThreads = 512, kS2OrderPer = 16;  // a tile of 8192 calls: keys held in registers
// keys NULL: by seeding hits (before s2a); else by s2a's sweep-work estimate per launch position (before
// the sweep: the hits inside the active ranges, which a spurious far diagonal can multiply several-fold
// at the same hit count), 64 buckets per doubling.
__global__ __launch_bounds__(kS2OrderThreads) void s2_order_kernel(const DevStage2Problem* __restrict__ probs, int n,
                                                                   const gmapdp_oligo_result* __restrict__ ores,
                                                                   unsigned long long* __restrict__ counters,
                                                                   const int* __restrict__ work) {
  __shared__ int hist[1024];
  __shared__ int wsum[16];
  int* order = reinterpret_cast<int*>(counters + 4);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int b = t; b < 1024; b += kS2OrderThreads) hist[b] = 0;
  __syncthreads();
  constexpr int kTile = kS2OrderThreads * kS2OrderPer;
  // bucket: descending totalpositions, 4 per bucket; the loads of a tile are issued together
  auto keys = [&](int base, int* key) {
    int idx[kS2OrderPer];
#pragma unroll
    for (int j = 0; j < kS2OrderPer; j++) {
      const int i = base + j * kS2OrderThreads + t;
      idx[j] = i < n ? probs[i].index : -1;
    }
#pragma unroll
    for (int j = 0; j < kS2OrderPer; j++) {
      if (work) {
        const int i = base + j * kS2OrderThreads + t;
        const int K = i < n ? max(work[i], 0) : 0;
        key[j] = idx[j] >= 0 ? 1023 - min((int)(64.0f * __log2f((float)K + 1.0f)), 1023) : -1;
      } else {
        const int T = idx[j] >= 0 ? ores[idx[j]].totalpositions : 0;
        key[j] = idx[j] >= 0 ? 1023 - min(max(T, 0) >> 2, 1023) : -1;
      }
    }
  };
  for (int base = 0; base < n; base += kTile) {
    int key[kS2OrderPer];
    keys(base, key);
#pragma unroll
    for (int j = 0; j < kS2OrderPer; j++)
      if (key[j] >= 0) atomicAdd(&hist[key[j]], 1);
  }
  __syncthreads();
  // exclusive prefix over the 1024 buckets, two per thread
  const int v0 = hist[2 * t], v1 = hist[2 * t + 1];
  const int incl = wave_incl_sum(v0 + v1, lane);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int off = 0;
  for (int k = 0; k < w; k++) off += wsum[k];
  __syncthreads();
  hist[2 * t] = off + incl - v0 - v1;
  hist[2 * t + 1] = off + incl - v1;
  __syncthreads();
  for (int base = 0; base < n; base += kTile) {
    int key[kS2OrderPer];
    keys(base, key);
#pragma unroll
    for (int j = 0; j < kS2OrderPer; j++)
      if (key[j] >= 0) order[atomicAdd(&hist[key[j]], 1)] = base + j * kS2OrderThreads + t;
  }
}

// kMirror: a Stage2_compute_starts call (GMAPDP_S2X_STARTS).  Its sweep, align_compute_scores_lookforward
// (stage2.c:4610), is the lookback sweep on the mirrored call: query position q -> nq - 1 - q, hit h of n ->
// n - 1 - h, chrpos p -> M - p with M = chrinit + chrterm (every hit lies in [chrinit, chrterm], so M - p does
// too: ascending within a mirrored position, below 2^31).  In the flat hit index that is i -> N - 1 - i.  The
// layout below writes the mirrored call -- maps, off[], rmap, the first swept position's range, and the
// per-position hit counts (npq' in the maxactive array, which nothing reads after this kernel) -- and
// s2b_starts_kernel runs the ENDS sweep on it unchanged; s2c_kernel<.., .., 3> un-mirrors.
template <bool kMirror>
__device__ __forceinline__ void s2a_body(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap, int* sh) {
  const int lane = threadIdx.x;
  const int pos = s2_problem(counters);
  const DevStage2Problem P = probs[pos];
  // the sweep-work estimate of this launch position (s2_order_kernel re-orders the sweep by it)
  int* work = reinterpret_cast<int*>(counters + 4) + gridDim.x;
  if (lane == 0) work[pos] = 0;
  const int ql = P.querylength, nq = ql - kS2K + 1;
  const gmapdp_oligo_result O = ores[P.index];
  const int T = O.totalpositions, nd = O.ndiagonals;
  const int32_t* npq = npos_all + P.qoff;
  const int32_t* mpq = map_all + P.qoff;
  const S2Scratch so = s2_scratch(ql, T, nd);
  unsigned char* S = scratch + P.scratch_offset;
  int* diff = reinterpret_cast<int*>(S + so.diff);
  double* run = reinterpret_cast<double*>(S + so.run);
  int* off = reinterpret_cast<int*>(S + so.off);
  uint32_t* minact = reinterpret_cast<uint32_t*>(S + so.minact);
  uint32_t* maxact = reinterpret_cast<uint32_t*>(S + so.maxact);
  int* first = reinterpret_cast<int*>(S + so.first);
  int* proc = reinterpret_cast<int*>(S + so.proc);
  S2Diag* dg = reinterpret_cast<S2Diag*>(S + so.diags);
  int* ord = reinterpret_cast<int*>(S + so.ord);
  int* tmp = reinterpret_cast<int*>(S + so.tmp);
  S2Hit* hits = reinterpret_cast<S2Hit*>(S + so.hits);
  int* cand = reinterpret_cast<int*>(S + so.cand);
  int* keep = reinterpret_cast<int*>(S + so.keep);
  S2Path* pth = reinterpret_cast<S2Path*>(S + so.paths);
  int* pathq = reinterpret_cast<int*>(S + so.pq);
  int* pathh = reinterpret_cast<int*>(S + so.ph);
  int* sbuf = reinterpret_cast<int*>(S + so.sbuf);
  (void)sh; (void)diff; (void)run; (void)off; (void)minact; (void)maxact; (void)first; (void)proc; (void)dg;
  (void)ord; (void)tmp; (void)hits; (void)cand; (void)keep; (void)pth; (void)pathq; (void)pathh; (void)sbuf;
  (void)npq; (void)mpq; (void)nq; (void)blocks; (void)nwords; (void)qseq; (void)quc; (void)table_all;
  (void)diag_all; (void)counters; (void)scratch_cap; (void)paths_out; (void)path_cap; (void)pairs_out; (void)pair_cap;
  gmapdp_stage2_result R;
  R.nresults = 0;
  R.npaths = 0;
  R.ncovered = 0;
  R.status = kS2NoPositions;
  R.diag_querystart = R.diag_queryend = 0;
  R.path_offset = 0;
  R.npairs = 0;
  S2_MARK(0);
  // chaining scratch too small, or the seeding's event pool could not take the call (oned_matrix_p -1)
  if (P.scratch_offset + (unsigned long long)so.total > scratch_cap || O.oned_matrix_p < 0) {
    if (lane == 0) {
      R.status = kS2Overflow;
      results[P.index] = R;
    }
    return;
  }

  // ---- Diag_update_coverage: depth per query position from a difference array ----
  for (int q = lane; q <= ql; q += 64) diff[q] = 0;
  for (int d = lane; d < nd; d += 64) {
    const int32_t* r = diag_all + 4 * (O.diag_offset + d);
    S2Diag x;
    x.diagonal = (uint32_t)r[0];
    x.querystart = r[1];
    x.queryend = r[2];
    x.nconsecutive = r[3];
    x.dominatedp = 0;
    x.pad_ = 0;
    x.score = 0.0;
    dg[d] = x;
  }
  wave_sync();
  for (int d = lane; d < nd; d += 64) {
    atomicAdd(&diff[dg[d].querystart], 1);
    atomicAdd(&diff[dg[d].queryend], -1);
  }
  wave_sync();
  int carry = 0, ncovered = 0;
  for (int cb = 0; cb < ql; cb += 64) {
    const int q = cb + lane;
    const int v = q < ql ? diff[q] : 0;
    const int depth = carry + wave_incl_sum(v, lane);
    carry = __shfl(depth, 63, 64);
    ncovered += wave_sum_i(q < ql && depth > 0 ? 1 : 0);
    if (q < ql) run[q] = depth > 0 ? 1.0 / (double)depth : 0.0;  // assign_scores' per-position term
  }
  R.ncovered = ncovered;
  const double pct = (double)ncovered / (double)ql;
  if (T == 0) {
    R.status = kS2NoPositions;
  } else if (P.kind == 0 && ql > 150 && pct < 0.3 && ncovered < 200) {  // (_one / _ends: totalpositions alone)
    R.status = kS2Coverage;
  } else {
    R.status = kS2Chained;
  }
  if (R.status != kS2Chained) {
    if (lane == 0) results[P.index] = R;
    return;
  }
  wave_sync();

  S2_MARK(1);
  // ---- Diag_compute_bounds ----
  const uint32_t chrinit = P.plusp ? P.chrstart : (P.chrhigh - P.chroffset) - P.chrend;
  const uint32_t chrterm = P.plusp ? P.chrend : (P.chrhigh - P.chroffset) - P.chrstart;
  const uint32_t genomiclength = P.chrend - P.chrstart;
  int qstart, qend;
  if (nd == 0 || P.kind != 0) {  // no diagonals; Stage2_compute_one / _ends: Diag_max_bounds (diag.c:894)
    fill_range(lane, minact, 0, ql - 1, [&](int) { return chrinit; });
    fill_range(lane, maxact, 0, ql - 1, [&](int) { return chrterm; });
    qstart = 0;
    qend = ql - 1;
  } else {
    // assign_scores: running sum in query order, sequential as the reference rounds it, but fed from
    // registers: 64 terms per coalesced load, added one by one in order by every lane alike (the same
    // IEEE sums), lane j keeping the prefix through term j (one lane walking run[] took a global round trip
    // per query position)
    {
      double acc = 0.0;
      for (int cb = 0; cb < ql; cb += 64) {
        const int q = cb + lane;
        const double v = q < ql ? run[q] : 0.0;
        const int2 vi = *reinterpret_cast<const int2*>(&v);
        double pre = 0.0;
        const int m = ql - cb < 64 ? ql - cb : 64;
        for (int j = 0; j < m; j++) {
          int2 t;
          t.x = __builtin_amdgcn_readlane(vi.x, j);
          t.y = __builtin_amdgcn_readlane(vi.y, j);
          acc += *reinterpret_cast<const double*>(&t);
          if (lane == j) pre = acc;
        }
        if (q < ql) run[q] = pre;
      }
    }
    wave_sync();
    for (int d = lane; d < nd; d += 64) dg[d].score = run[dg[d].queryend] - run[dg[d].querystart];
    wave_sync();
    // gooddiagonals (List_push: reverse list order), else all in list order
    int ngood = 0;
    for (int cb = 0; cb < nd; cb += 64) {
      const int d = nd - 1 - (cb + lane);
      const bool g = (cb + lane < nd) && dg[d].score >= 10.0;
      const uint64_t m = ballot(g);
      if (g) ord[ngood + lanes_below(m, lane)] = d;
      ngood += __popcll(m);
    }
    if (ngood == 0) {
      for (int d = lane; d < nd; d += 64) ord[d] = d;
      ngood = nd;
    }
    wave_sync();
    // compute_dominance: stable sort by nconsecutive descending, then drop dominated diagonals
    wave_sort(lane, ngood, ord, tmp, sbuf, [&](int a, int b) { return dg[a].nconsecutive > dg[b].nconsecutive; });
    int nunique = ngood;
    for (int i = 0; i < nunique; i++) {
      const S2Diag sup = dg[tmp[i]];
      const int expected = sup.queryend + 1 - sup.querystart;
      int threshold;
      if (expected < 100 && sup.nconsecutive > expected - 10) {
        threshold = sup.nconsecutive - 20;
      } else if (expected >= 100 && sup.nconsecutive > expected * 0.90) {
        threshold = (int)(sup.nconsecutive * 0.80);
      } else {
        continue;
      }
      int k = i + 1;
      for (int cb = i + 1; cb < nunique; cb += 64) {
        const int j = cb + lane;
        int d = -1;
        bool live = false;
        if (j < nunique) {
          d = tmp[j];
          S2Diag& sub = dg[d];
          if (sub.querystart >= sup.querystart && sub.queryend <= sup.queryend && sub.nconsecutive < threshold)
            sub.dominatedp = 1;
          live = !sub.dominatedp;
        }
        const uint64_t m = ballot(live);
        wave_sync();
        if (live) tmp[k + lanes_below(m, lane)] = d;
        k += __popcll(m);
        wave_sync();
      }
      nunique = k;
    }
    // stable sort by diagonal
    wave_sort(lane, nunique, tmp, ord, sbuf, [&](int a, int b) { return dg[a].diagonal < dg[b].diagonal; });
    if (nunique > 100) {  // keep_center_diagonal
      if (lane == 0) {
        const uint32_t mind = dg[ord[0]].diagonal, maxd = dg[ord[nunique - 1]].diagonal;
        const int nbins = (int)((maxd - mind) / 10000) + 1;
        // bins by a sweep over the sorted diagonals (bin index is monotone in the order)
        int maxcount = 0, curbin = -1, curcount = 0;
        uint32_t center = 0;
        for (int i = 0; i <= nunique; i++) {
          const int b = i < nunique ? (int)((dg[ord[i]].diagonal - mind) / 10000) : nbins;
          if (b != curbin) {
            if (curbin >= 0 && curcount > maxcount) {
              maxcount = curcount;
              center = mind + 10000u * (uint32_t)curbin;
            }
            curbin = b;
            curcount = 0;
          }
          curcount++;
        }
        center += 5000;
        int j = 0;
        for (int i = 0; i < nunique; i++) {
          const uint32_t dd = dg[ord[i]].diagonal;
          if (!(dd + 10000 < center || dd > center + 10000)) ord[j++] = ord[i];
        }
        sh[0] = j;
      }
      wave_sync();
      nunique = sh[0];
    }
    const S2Diag d0 = dg[ord[0]], dl = dg[ord[nunique - 1]];
    qstart = ql - 1;
    qend = 0;
    {
      int mn = ql - 1, mx = 0;
      for (int i = lane; i < nunique; i += 64) {
        mn = min(mn, dg[ord[i]].querystart);
        mx = max(mx, dg[ord[i]].queryend);
      }
      qstart = -wave_max_i(-mn);
      qend = wave_max_i(mx);
    }
    auto minline = [&](uint32_t diagonal) {
      return [=](int q) {
        return (diagonal + (uint32_t)q < (uint32_t)kS2ExtraBounds) ? chrinit
                                                                    : chrinit + diagonal + (uint32_t)q - kS2ExtraBounds;
      };
    };
    auto maxline = [&](uint32_t diagonal) {
      return [=](int q) {
        const uint32_t position = diagonal + (uint32_t)q + kS2ExtraBounds;
        return (position > genomiclength) ? chrterm : chrinit + position;
      };
    };
    // minactive
    fill_range(lane, minact, 0, d0.querystart - 1, [&](int) { return 0u; });
    int q = d0.querystart;
    uint32_t diagonal = d0.diagonal;
    fill_range(lane, minact, q, d0.queryend, minline(diagonal));
    q = max(q, d0.queryend + 1);
    for (int i = 0, j; i < nunique; i = j) {
      const int qe_i = dg[ord[i]].queryend;
      for (j = i + 1; j < nunique && dg[ord[j]].queryend <= qe_i; j++) ;
      if (j < nunique) {
        diagonal = dg[ord[i]].diagonal;
        const int b = dg[ord[j]].queryend;
        fill_range(lane, minact, q, b, minline(diagonal));
        q = max(q, b + 1);
      }
    }
    {
      const uint32_t dlast = diagonal;
      fill_range(lane, minact, q, ql - 1, [=](int qq) {
        return (dlast + (uint32_t)qq < (uint32_t)kS2ExtraBounds) ? chrinit : chrinit + (uint32_t)qq - kS2ExtraBounds;
      });
    }
    // maxactive
    const int activeend = dl.queryend;
    fill_range(lane, maxact, activeend + 1, ql - 1, [&](int) { return chrterm; });
    q = min(ql - 1, activeend);
    diagonal = dl.diagonal;
    fill_range(lane, maxact, dl.querystart, q, maxline(diagonal));
    q = min(q, dl.querystart - 1);
    for (int i = nunique - 1, j; i >= 0; i = j) {
      const int qs_i = dg[ord[i]].querystart;
      for (j = i - 1; j >= 0 && dg[ord[j]].querystart > qs_i; j--) ;
      if (j >= 0) {
        diagonal = dg[ord[i]].diagonal;
        const int a = dg[ord[j]].querystart;
        fill_range(lane, maxact, a, q, maxline(diagonal));
        q = min(q, a - 1);
      }
    }
    fill_range(lane, maxact, 0, q, maxline(diagonal));
  }
  R.diag_querystart = qstart;
  R.diag_queryend = qend;

  S2_MARK(2);
  // ---- per-hit arrays: the hits of query position q at hits[off[q] ...] (Linkmatrix_1d_new) ----
  // Only the hits the chaining can touch are laid out.  The sweep scores the hits of q inside [minactive,
  // maxactive] (stage2.c:3849-3857); a position's hits ascend in chrpos, so they are [low, high): low the
  // first hit with map >= minactive, high the first with map > max(maxactive, minactive - 1) (the search
  // from low: an empty range when maxactive < minactive).  revise_active_lookback (:4070) rebuilds the
  // active list from that range alone before any later position looks back, so a hit outside it is never a
  // lookback target, and its fwd_score stays 0: never a cell (get_cells_fwd :3450), never on a path.  The
  // one exception is q0, the first position with hits at or after querystart: the reference gives every
  // hit of it fwd_score = indexsize (:3792-3815), so the ones outside the range are cells of score 8, which
  // reach the paths of a call whose best score is below 8 + FINAL_SCORE_TOLERANCE.  q0 therefore keeps all
  // its hits, and its range goes to the sweep beside the arrays (fp[0], fp[1]); every other position's
  // range is its whole compact slice.
  //
  // 64 positions at a time, each lane its position's range in its table slice (one round of loads for a
  // slice of <= 4 hits, else two binary searches); the offsets by a prefix scan of the counts; then the
  // hits written in hit order, lane l taking hit base + l (its position the last lane whose offset is <=
  // the hit, a binary search over the lanes), so each store instruction covers 64 consecutive hits.
  // rmap[q]: the first hit of q's range (0: none).  The sweep's chunk metadata is one round of
  // independent loads.
  int* fp = reinterpret_cast<int*>(S + so.lh);
  uint32_t* mapsa = reinterpret_cast<uint32_t*>(S + so.maps);
  int* sca = reinterpret_cast<int*>(S + so.sc);
  uint32_t* rmapa = reinterpret_cast<uint32_t*>(diff);  // (the coverage is done with diff)
  const uint32_t* __restrict__ tb = table_all + O.table_offset;  // (mappings relative to the call's table)
  wave_sync();
  // (kMirror: q runs over the mirrored positions, qr the real one whose seeding is read; qstart 0, qend ql - 1)
  const uint32_t mirror = chrinit + chrterm;
  int* npm = reinterpret_cast<int*>(maxact);  // kMirror: the hit counts in mirrored order, for the sweep
  (void)mirror; (void)npm;
  int q0 = -1;
  for (int cb = qstart & ~63; cb <= qend && q0 < 0; cb += 64) {
    const int q = cb + lane;
    const int qr = kMirror ? nq - 1 - q : q;
    const uint64_t m = ballot(q >= qstart && q <= qend && q < nq && npq[qr] > 0);
    if (m) q0 = cb + __ffsll((long long)m) - 1;
  }
  // chromosome positions past 2^31 (Pairpool_push would drop them: outside the domain) are looked for among
  // all the seeded hits, as before the compact layout: none when the window ends below 2^31 (a hit is
  // chrinit + an offset within the window), else each position's last (largest) hit is read
  const bool scan_big = (uint64_t)chrinit + (uint64_t)genomiclength + (uint64_t)ql + 64u >= 0x80000000ull;
  carry = 0;
  bool big = false;
  int wk = 0;
  for (int cb = 0; cb < ql; cb += 64) {
    const int q = cb + lane;
    const int qr = kMirror ? nq - 1 - q : q;
    const int v = q < nq ? npq[qr] : 0;
    const int mq = v > 0 ? mpq[qr] : 0;
    const bool act = q <= qend && v > 0;
    // (kMirror: Diag_max_bounds' constants; maxact is being overwritten with npm)
    const uint32_t qmn = act ? (kMirror ? chrinit : minact[q]) : 0u, qmx0 = act ? (kMirror ? chrterm : maxact[q]) : 0u;
    const uint32_t qmx = (qmn > 0 && qmx0 < qmn - 1) ? qmn - 1 : qmx0;
    if (scan_big && v > 0) big |= (tb[mq + v - 1] >= 0x80000000u);
    int low = 0, high = 0;
    uint32_t rmap = 0u;
    if (act) {
      const uint32_t* __restrict__ sl = tb + mq;
      if (v <= 4) {
        uint32_t e[4];
#pragma unroll
        for (int k = 0; k < 4; k++) e[k] = k < v ? sl[k] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          low += (k < v && e[k] < qmn) ? 1 : 0;
          high += (k < v && e[k] <= qmx) ? 1 : 0;
        }
        high = max(high, low);
        const uint32_t el = low == 0 ? e[0] : low == 1 ? e[1] : low == 2 ? e[2] : e[3];
        rmap = high > low ? el : 0u;
      } else {
        int lo = 0, hi = v;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (sl[mid] < qmn) lo = mid + 1;
          else hi = mid;
        }
        low = lo;
        hi = v;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (sl[mid] <= qmx) lo = mid + 1;
          else hi = mid;
        }
        high = lo;
        rmap = high > low ? sl[low] : 0u;
      }
    }
    // the sweep's work: a position's lookbacks grow with the hits of its range (each one beyond the first
    // a full lookback); a diagonal far from the others widens those ranges over the gap
    if (q >= qstart && q <= qend && high > low) wk += 1 + 4 * (high - low - 1);
    if constexpr (kMirror) rmap = high > low ? mirror - tb[mq + high - 1] : 0u;  // the mirrored range's first hit
    int c = high - low, first_hit = mq + low;
    if (q == q0) {  // (act: q0 <= qend and it has hits)
      fp[0] = kMirror ? v - high : low;
      fp[1] = kMirror ? v - low : high;
      c = v;
      first_hit = mq;
    }
    const int incl = carry + wave_incl_sum(c, lane);
    const int o = incl - c;
    if (q < ql) {
      off[q] = o;
      rmapa[q] = rmap;
      if constexpr (kMirror) npm[q] = v;
    }
    const int hend = __shfl(incl, 63, 64);
    for (int base = carry; base < hend; base += 64) {
      const int h = base + lane;
      int j = 0;
#pragma unroll
      for (int st = 32; st >= 1; st >>= 1) {
        const int oj = __shfl(o, j + st, 64);
        if (oj <= h) j += st;
      }
      const int oq = __shfl(o, j, 64), fj = __shfl(first_hit, j, 64);
      if constexpr (kMirror) {  // the position's laid-out hits last first, each M - chrpos
        const int cj = __shfl(c, j, 64);
        if (h < hend) {
          mapsa[h] = mirror - tb[fj + (cj - 1 - (h - oq))];
          sca[h] = 0;
        }
      } else if (h < hend) {
        mapsa[h] = tb[fj + (h - oq)];
        sca[h] = 0;
      }
    }
    carry = hend;
  }
  if (lane == 0) off[ql] = carry;  // the hits laid out (<= T)
  // zeroed records only for the calls s2c walks through its LDS link table (its loader reads every
  // record); the others keep just the chrpos and a zero score per hit (the sweep writes what it scores)
  if (s2c_lds_class(T, carry, nq))
    for (int h = lane; h < carry; h += 64) hits[h] = S2Hit{0, 0, 0, 0};  // CALLOC (a zero link: position 0's hit 0)
  if (ballot(big)) {  // chromosome positions past 2^31: Pairpool_push would drop them (outside the domain)
    if (lane == 0) {
      R.status = kS2Domain;
      results[P.index] = R;
    }
    return;
  }
  wave_sync();
  wk = wave_sum_i(wk);
  if (lane == 0) work[pos] = wk;

  if (lane == 0) results[P.index] = R;  // status 2 with the query bounds: the sweep and the paths follow
}

__global__ __launch_bounds__(64) void s2a_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap) {
  __shared__ int sh[8];
  s2a_body<false>(probs, blocks, nwords, qseq, quc, ores, npos_all, map_all, table_all, diag_all, scratch, counters,
                  scratch_cap, results, paths_out, path_cap, pairs_out, pair_cap, sh);
}
// the mirrored layout of a GMAPDP_S2X_STARTS batch, in a kernel of its own so that s2a_kernel keeps its registers
__global__ __launch_bounds__(64) void s2a_starts_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap) {
  __shared__ int sh[8];
  s2a_body<true>(probs, blocks, nwords, qseq, quc, ores, npos_all, map_all, table_all, diag_all, scratch, counters,
                 scratch_cap, results, paths_out, path_cap, pairs_out, pair_cap, sh);
}

// the lookback sweep (align_compute_scores_lookback) of the calls s2a_kernel left chained
#ifndef GMAPDP_S2B_WPE
#define GMAPDP_S2B_WPE 4  // waves per SIMD the sweep's registers are budgeted for (variants: make variant DEFS=...)
#endif
// (the body of both instantiations: s2b_kernel, the default, and s2b_canon_kernel, which also takes the
// MaxEnt tables)
template <bool kCanon, int kKind = 0>
__device__ __forceinline__ void s2b_body(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap,
    const double* __restrict__ metab) {
  __shared__ int sh[8];
  const int lane = threadIdx.x;
  const DevStage2Problem P = probs[s2_problem(counters)];
  const int ql = P.querylength, nq = ql - kS2K + 1;
  const gmapdp_oligo_result O = ores[P.index];
  const int T = O.totalpositions, nd = O.ndiagonals;
  const int32_t* npq = npos_all + P.qoff;
  const int32_t* mpq = map_all + P.qoff;
  const S2Scratch so = s2_scratch(ql, T, nd);
  unsigned char* S = scratch + P.scratch_offset;
  int* diff = reinterpret_cast<int*>(S + so.diff);
  double* run = reinterpret_cast<double*>(S + so.run);
  int* off = reinterpret_cast<int*>(S + so.off);
  uint32_t* minact = reinterpret_cast<uint32_t*>(S + so.minact);
  uint32_t* maxact = reinterpret_cast<uint32_t*>(S + so.maxact);
  int* first = reinterpret_cast<int*>(S + so.first);
  int* proc = reinterpret_cast<int*>(S + so.proc);
  S2Diag* dg = reinterpret_cast<S2Diag*>(S + so.diags);
  int* ord = reinterpret_cast<int*>(S + so.ord);
  int* tmp = reinterpret_cast<int*>(S + so.tmp);
  S2Hit* hits = reinterpret_cast<S2Hit*>(S + so.hits);
  int* cand = reinterpret_cast<int*>(S + so.cand);
  int* keep = reinterpret_cast<int*>(S + so.keep);
  S2Path* pth = reinterpret_cast<S2Path*>(S + so.paths);
  int* pathq = reinterpret_cast<int*>(S + so.pq);
  int* pathh = reinterpret_cast<int*>(S + so.ph);
  int* sbuf = reinterpret_cast<int*>(S + so.sbuf);
  (void)sh; (void)diff; (void)run; (void)off; (void)minact; (void)maxact; (void)first; (void)proc; (void)dg;
  (void)ord; (void)tmp; (void)hits; (void)cand; (void)keep; (void)pth; (void)pathq; (void)pathh; (void)sbuf;
  (void)npq; (void)mpq; (void)nq; (void)blocks; (void)nwords; (void)qseq; (void)quc; (void)table_all;
  (void)diag_all; (void)counters; (void)scratch_cap; (void)paths_out; (void)path_cap; (void)pairs_out; (void)pair_cap;
  const gmapdp_stage2_result R0 = results[P.index];
  if (R0.status != kS2Chained) return;
  const int qstart = R0.diag_querystart, qend = R0.diag_queryend;
  S2_MARK(3);
#ifdef GMAPDP_OI_TIMING
  const unsigned long long tw0 = wall_clock64();
#endif
  // ---- align_compute_scores_lookback: the sweep on lane 0 ----
  {
    S2WT<kCanon, kKind < 2, kKind < 2, kKind == 0> W;  // (kind 3, STARTS: ENDS' facts on the mirrored call)
    if constexpr (kCanon) {
      W.blocks = blocks;
      W.metab = metab;
      W.nwords = nwords;
      W.chroffset = P.chroffset;
      W.chrhigh = P.chrhigh;
      W.plusp = P.plusp;
      for (unsigned& c : W.nform) c = 0;
      W.nmult[0] = W.nmult[1] = W.nevals = 0;
      W.in_mult = 0;
    }
    W.hits = hits;
    W.maps = reinterpret_cast<const uint32_t*>(S + so.maps);
    W.sc = reinterpret_cast<int*>(S + so.sc);
    W.off = off;
    W.actn = first;
    W.alist = keep;
    W.pq = proc;
    W.pn = pathq;
    W.poff = pathh;
    W.pstart = reinterpret_cast<int*>(run);
    W.pushed = 0;
    W.tracectr = 0;
    W.splicingp = P.splicingp;
    W.lane = lane;
    W.maxintronlen = P.maxintronlen;
    // (kind 3: the hit counts in mirrored order, which s2a_starts_kernel left in the maxactive array)
    const int32_t* npw = kKind == 3 ? reinterpret_cast<const int32_t*>(maxact) : npq;
    s2_sweep(W, npw, nq, reinterpret_cast<const int*>(S + so.lh), reinterpret_cast<const uint32_t*>(diff), qstart,
             qend);  // q0's range / rmap (s2a_kernel)
    if constexpr (kCanon) {
      for (int f = 0; f < 8; f++) {
        const unsigned mine = f < 5 ? W.nform[f] : f < 7 ? W.nmult[f - 5] : W.nevals;
        const int all = wave_sum_i((int)mine);
        if (lane == 0 && all) atomicAdd(&g_s2_canon[f], (unsigned long long)all);
      }
    }
  }
  wave_sync();
#ifdef GMAPDP_OI_TIMING
  if (lane == 0 && P.index < 16384) {  // by call
    g_s2_wave[0][P.index] = (unsigned int)(wall_clock64() - tw0);
    g_s2_wave[1][P.index] = (unsigned int)(qend - qstart + 1);
    g_s2_wave[2][P.index] = (unsigned int)T;
  }
#endif

  S2_MARK(4);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GMAPDP_S2B_WPE))) void s2b_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap) {
  s2b_body<false>(probs, blocks, nwords, qseq, quc, ores, npos_all, map_all, table_all, diag_all, scratch, counters,
                  scratch_cap, results, paths_out, path_cap, pairs_out, pair_cap, nullptr);
}

// the cross-species sweep (GMAPDP_S2_CANONICAL_MIDDLE): the same arguments, then the MaxEnt tables
// (budgeted for 2 waves per SIMD: 178 VGPRs without scratch; at 3 and 4 the predicate's windows and the FP64
// products spill, 16 and 112 bytes per lane)
#ifndef GMAPDP_S2B_CANON_WPE
#define GMAPDP_S2B_CANON_WPE 2
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GMAPDP_S2B_CANON_WPE))) void s2b_canon_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap,
    const double* __restrict__ metab) {
  s2b_body<true>(probs, blocks, nwords, qseq, quc, ores, npos_all, map_all, table_all, diag_all, scratch, counters,
                 scratch_cap, results, paths_out, path_cap, pairs_out, pair_cap, metab);
}

// the sweeps of Stage2_compute_one (localp, middlep, no repetitive-position skipping) and Stage2_compute_ends
// (neither localp nor middlep, no skipping): S2WT's three facts; short calls, so no register budget of their own
__global__ __launch_bounds__(64) void s2b_one_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap) {
  s2b_body<false, 1>(probs, blocks, nwords, qseq, quc, ores, npos_all, map_all, table_all, diag_all, scratch, counters,
                     scratch_cap, results, paths_out, path_cap, pairs_out, pair_cap, nullptr);
}
__global__ __launch_bounds__(64) void s2b_ends_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap) {
  s2b_body<false, 2>(probs, blocks, nwords, qseq, quc, ores, npos_all, map_all, table_all, diag_all, scratch, counters,
                     scratch_cap, results, paths_out, path_cap, pairs_out, pair_cap, nullptr);
}
// Stage2_compute_starts: align_compute_scores_lookforward as the ENDS sweep over s2a_starts_kernel's mirrored layout
__global__ __launch_bounds__(64) void s2b_starts_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap) {
  s2b_body<false, 3>(probs, blocks, nwords, qseq, quc, ores, npos_all, map_all, table_all, diag_all, scratch, counters,
                     scratch_cap, results, paths_out, path_cap, pairs_out, pair_cap, nullptr);
}

// traceback_one over the LDS link table, 8 B per hit: lql[i] = query position << 16 | a bit 15 set when
// the hit has fewer than MIN_TERMINAL_NCONSECUTIVE consecutive matches | the predecessor's hit index
// (0x7fff: none); map[i] its chrpos.  Calls with more hits or query positions past 2^16 walk the global
// arrays instead.
constexpr uint32_t kS2NoPred = 0x7fffu;
// The walk runs on the whole wave: a link to the previous hit index (consecutive query positions with
// one hit each, the common case) continues a run, so each step takes the run of up to 64 nodes from gi
// down (one LDS read per lane, a ballot for the run's end) instead of one dependent LDS read per node.
// Visited nodes (chrpos < 2^31) are numbered in walk order; pq/ph (optional) receive their query and
// genomic positions.  Returns the count and the first and last visited nodes (wave-uniform).
struct S2WalkOut {
  int n, top, bottom;
};
// The same walk over the global hit arrays, for calls with more hits than the LDS link table holds (a
// 214-kb window's random matches: ~4 hits per query position, so a path's nodes are not consecutive hit
// indices and s2_walk_wave would advance one node per step).  A path mostly follows one diagonal through
// consecutive query positions, so each step guesses the next 64 nodes there: lane k takes the hit of
// position q - k with map - k (a binary search in that position's hits, which ascend), and the guesses
// hold while each one is its predecessor's link; the walk goes on from the last holding node's real link.
// A node's query position is not stored: the guesses know theirs, and after a real link it is first
// taken to continue the run (the position before the last node's, checked against off[] by the loads the
// guesses make anyway), else found by one wave search of off[].  Same nodes, order and outputs as s2_walk.
__device__ S2WalkOut s2_walk_diag(const S2Hit* __restrict__ hits, const uint32_t* __restrict__ maps,
                                  const int* __restrict__ scs, const int* __restrict__ off, int ql, int gi, int lane,
                                  int* __restrict__ pq, int* __restrict__ ph) {
  S2WalkOut o = {0, -1, -1};
  while (gi >= 0 && hits[gi].consec < kS2MinTerminal) gi = hits[gi].pred;  // prune the 3' end
  int qn = -1;  // gi's query position (-1: not known)
  while (gi >= 0) {
    if (qn < 0) qn = s2_hit_pos_wave(off, ql, gi, lane);
    int p = qn - lane;
    int lo = p >= 0 ? off[p] : 0, hi = p >= 0 ? off[p + 1] : 0;
    if (!(s2_u(lo) <= gi && gi < s2_u(hi))) {  // the link left the run of positions
      qn = s2_hit_pos_wave(off, ql, gi, lane);
      p = qn - lane;
      lo = p >= 0 ? off[p] : 0;
      hi = p >= 0 ? off[p + 1] : 0;
    }
    const uint32_t mn = s2_u(maps[gi]);
    const uint32_t target = mn - (uint32_t)lane;
    int idx = -1;
    if (lane == 0) {
      idx = gi;
    } else if (p >= 0) {
      const int end = hi;
      while (lo < hi) {  // (4 B per hit: a step's 64 searches touch ~1 KB, not the records' ~4 KB)
        const int mid = (lo + hi) >> 1;
        if (maps[mid] < target) lo = mid + 1;
        else hi = mid;
      }
      if (lo < end && maps[lo] == target) idx = lo;
    }
    // a guess the sweep never scored (score 0) is on no path, and its record was never written: it fails
    // (a path node's link always points at a scored hit, so such a guess could not hold anyway)
    int sc = 0;
    S2Hit x = {0, 0, 0, -1};
    if (idx >= 0) {  // (both loads issued together; an unwritten record is read and dropped)
      sc = scs[idx];
      x = hits[idx];
    }
    if (lane > 0 && sc <= 0) idx = -1;
    const int pred = idx >= 0 ? x.pred : -1;
    const uint32_t mx = idx >= 0 ? target : 0x80000000u;  // (the node's chrpos: mn, or the guess it matched)
    const int qx = p;
    // node k holds when node k - 1 does and node k - 1's link is this guess
    const int prev_pred = __shfl_up(pred, 1, 64);
    const bool c = lane == 0 || (idx >= 0 && prev_pred == idx);
    const uint64_t brk = ballot(!c);
    const int len = brk ? __ffsll((long long)brk) - 1 : 64;  // nodes 0 .. len-1
    const bool vis = lane < len && (int)mx >= 0;
    const uint64_t vm = ballot(vis);
    if (vis && pq) {
      const int k = o.n + lanes_below(vm, lane);
      pq[k] = qx;
      ph[k] = (int)mx;
    }
    if (vm) {
      const int f = __ffsll((long long)vm) - 1, l = 63 - __clzll((long long)vm);
      if (o.top < 0) o.top = __builtin_amdgcn_readlane(idx, f);
      o.bottom = __builtin_amdgcn_readlane(idx, l);
    }
    o.n += __popcll(vm);
    gi = __builtin_amdgcn_readlane(pred, len - 1);
    qn = max(qn - len, -1);  // the position a continuing run would have (checked above)
  }
  return o;
}

__device__ S2WalkOut s2_walk_wave(const uint32_t* lql, const uint32_t* map, int gi, int lane, int* pq, int* ph) {
  S2WalkOut o = {0, -1, -1};
  uint32_t w = lql[gi];
  while (w & 0x8000u) {  // prune the 3' end
    const uint32_t pr = w & kS2NoPred;
    if (pr == kS2NoPred) return o;
    gi = (int)pr;
    w = lql[gi];
  }
  for (;;) {
    const int x = gi - lane;
    const uint32_t wx = x >= 0 ? lql[x] : kS2NoPred;
    const uint32_t px = wx & kS2NoPred;
    const bool cont = x >= 1 && px == (uint32_t)(x - 1);
    const uint64_t stop = ballot(!cont);
    const int r = stop ? __ffsll((long long)stop) - 1 : 63;  // lanes 0..r hold the run's nodes
    const uint32_t mx = lane <= r ? map[x] : 0x80000000u;
    const bool vis = (int)mx >= 0;
    const uint64_t vm = ballot(vis);
    if (vis && pq) {
      const int idx = o.n + lanes_below(vm, lane);
      pq[idx] = (int)(wx >> 16);
      ph[idx] = (int)mx;
    }
    if (vm) {
      if (o.top < 0) o.top = gi - (__ffsll((long long)vm) - 1);
      o.bottom = gi - (63 - __clzll((long long)vm));
    }
    o.n += __popcll(vm);
    const uint32_t pr = (uint32_t)__builtin_amdgcn_readlane((int)px, r);
    if (pr == kS2NoPred) return o;
    gi = (int)pr;
  }
}

// cells, traceback_one, Stage2_filter_unique, convert_to_nucleotides.  Two launches over the same order:
// kLdsWalk = false takes the calls whose link table does not fit LDS (more than kS2cCap hits: every 214-kb
// window) with no LDS reserved, so 6 waves per SIMD run (32 KB of LDS allowed 5 per CU); kLdsWalk = true
// takes the rest with the 32-KB link table.  The class goes by the seeding's hit count (s2c_lds_class), not
// by the fewer hits laid out: with the latter every 214-kb call fits the table, and the bench step was 2 ms
// slower at the table's 5 waves per CU.
// kModal: a cmet / atoi / ttoc context (convert_to_nucleotides outside STANDARD, stage2.c:5403-5452): every
// pair's genome character is the real (unreduced) genome's, and a pair whose query character differs from
// it carries ':' (AMBIGUOUS_COMP) instead of '|'.
// kKind: 0 Stage2_compute; GMAPDP_S2X_ONE (1) / _ENDS (2): the path loop with max_nalignments 1 (the best cell
// and every further cell of its score); ONE keeps the last path traced, with gap holders, its pairs 3' end first
// (List_reverse(middle), stage2.c:6908); ENDS converts every path without gap holders and filters the lists by
// Stage2pairs_filter_unique_ends (:6218); both add query_offset to the pairs' querypos.
// GMAPDP_S2X_STARTS (3), Stage2_compute_starts: the link records are those of the mirrored call (s2a_body).  The
// cells' keys are taken back to the real call (query position nq - 1 - q', root M - root' -- 0 stays the 0 the
// reference leaves in the first swept position's links -- and the hit order reversed), so get_cells_fwd's
// comparators see what the reference's see.  The walks follow the links as they are: in the real call from the
// cell towards the 3' end, pruning at the walk's start.  Their entries are then reversed and un-mirrored, which
// is the list convert_to_nucleotides receives (3'-most hit first); each list is written 3' end first
// (List_reverse(pairs), :7040), without gap holders, and the lists go through Stage2pairs_filter_unique_starts
// (:6114: chrend descending, then chrstart descending).
template <bool kLdsWalk, bool kModal, int kKind = 0>
__global__ __launch_bounds__(64) void s2c_kernel(
    const DevStage2Problem* __restrict__ probs, const uint32_t* __restrict__ blocks, uint64_t nwords,
    const char* __restrict__ qseq, const char* __restrict__ quc, const gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    const int32_t* __restrict__ diag_all, unsigned char* __restrict__ scratch, unsigned long long* __restrict__ counters,
    unsigned long long scratch_cap, gmapdp_stage2_result* __restrict__ results, gmapdp_path* __restrict__ paths_out,
    unsigned long long path_cap, gmapdp_path_pair* __restrict__ pairs_out, unsigned long long pair_cap) {
  __shared__ int sh[8];
  const int lane = threadIdx.x;
  const DevStage2Problem P = probs[s2_problem(counters)];
  const int ql = P.querylength, nq = ql - kS2K + 1;
  const gmapdp_oligo_result O = ores[P.index];
  const int T = O.totalpositions, nd = O.ndiagonals;
  const int32_t* npq = npos_all + P.qoff;
  const int32_t* mpq = map_all + P.qoff;
  const S2Scratch so = s2_scratch(ql, T, nd);
  unsigned char* S = scratch + P.scratch_offset;
  int* diff = reinterpret_cast<int*>(S + so.diff);
  double* run = reinterpret_cast<double*>(S + so.run);
  int* off = reinterpret_cast<int*>(S + so.off);
  uint32_t* minact = reinterpret_cast<uint32_t*>(S + so.minact);
  uint32_t* maxact = reinterpret_cast<uint32_t*>(S + so.maxact);
  int* first = reinterpret_cast<int*>(S + so.first);
  int* proc = reinterpret_cast<int*>(S + so.proc);
  S2Diag* dg = reinterpret_cast<S2Diag*>(S + so.diags);
  int* ord = reinterpret_cast<int*>(S + so.ord);
  int* tmp = reinterpret_cast<int*>(S + so.tmp);
  S2Hit* hits = reinterpret_cast<S2Hit*>(S + so.hits);
  const uint32_t* maps = reinterpret_cast<const uint32_t*>(S + so.maps);
  const int* scs = reinterpret_cast<const int*>(S + so.sc);
  int* cand = reinterpret_cast<int*>(S + so.cand);
  int* keep = reinterpret_cast<int*>(S + so.keep);
  S2Path* pth = reinterpret_cast<S2Path*>(S + so.paths);
  int* pathq = reinterpret_cast<int*>(S + so.pq);
  int* pathh = reinterpret_cast<int*>(S + so.ph);
  int* sbuf = reinterpret_cast<int*>(S + so.sbuf);
  (void)sh; (void)diff; (void)run; (void)off; (void)minact; (void)maxact; (void)first; (void)proc; (void)dg;
  (void)ord; (void)tmp; (void)hits; (void)cand; (void)keep; (void)pth; (void)pathq; (void)pathh; (void)sbuf;
  (void)npq; (void)mpq; (void)nq; (void)blocks; (void)nwords; (void)qseq; (void)quc; (void)table_all;
  (void)diag_all; (void)counters; (void)scratch_cap; (void)paths_out; (void)path_cap; (void)pairs_out; (void)pair_cap;
  gmapdp_stage2_result R = results[P.index];
  if (R.status != kS2Chained) return;
  if (s2c_lds_class(T, off[ql], nq) != kLdsWalk) return;  // the other launch's call
  S2_MARK(12);
  const int qstart = R.diag_querystart, qend = R.diag_queryend;
  // kind 3: M of the mirrored layout (s2a_body: chrinit + chrterm)
  const uint32_t mirror = (P.plusp ? P.chrstart : (uint32_t)((P.chrhigh - P.chroffset) - P.chrend)) +
                          (P.plusp ? P.chrend : (uint32_t)((P.chrhigh - P.chroffset) - P.chrstart));
  (void)mirror;
  // ---- get_cells_fwd + the path loop: cells within FINAL_SCORE_TOLERANCE of the best, each the best
  // of its root position, in (score desc, root asc, querypos desc, hit asc) order ----
  // one pass over the scores: the hits within the tolerance of the running best (a superset of those
  // within it of the final best, in hit order) with their scores, then the final best filters them
  const int h0 = off[qstart], h1 = off[qend + 1];
  // Per candidate slot: cand its hit, keep its score, cq its query position, croot its root, so the sorts
  // below compare slots with one load per key.  The path records' room (written from the walks on) holds
  // the last two and the two slot lists.
  const int H = T > 0 ? T : 1;
  int* cq = reinterpret_cast<int*>(pth);
  int* croot = cq + H;
  int* slots = croot + H;
  int* sorted = slots + H;
  int best = 0, ncand = 0;
  {
    // eight 64-hit chunks of the scores per step, loaded before any use: one round trip per 512 hits
    const int* __restrict__ scr = scs;
    int* __restrict__ cw = cand;
    int* __restrict__ kw = keep;
    constexpr int kB = 8;
    for (int cb = h0; cb < h1; cb += 64 * kB) {
      int sc[kB];
#pragma unroll
      for (int k = 0; k < kB; k++) {
        const int gi = cb + 64 * k + lane;
        sc[k] = gi < h1 ? scr[gi] : 0;  // (the compact score array: unscored hits hold 0)
      }
#pragma unroll
      for (int k = 0; k < kB; k++) {
        const int gi = cb + 64 * k + lane;
        best = max(best, wave_max_i(sc[k]));
        const bool c = gi < h1 && sc[k] > best - kS2FinalTolerance && sc[k] > 0;
        const uint64_t m = ballot(c);
        if (c) {
          cw[ncand + lanes_below(m, lane)] = gi;
          kw[ncand + lanes_below(m, lane)] = sc[k];
        }
        ncand += __popcll(m);
      }
    }
  }
  wave_sync();
  if (best > 0) {
    int n2 = 0;
    for (int cb = 0; cb < ncand; cb += 64) {
      const int i = cb + lane;
      const int gi = i < ncand ? cand[i] : 0, sc = i < ncand ? keep[i] : 0;
      const bool c = i < ncand && sc > best - kS2FinalTolerance;
      const uint64_t m = ballot(c);
      if (c) {  // in place: n2 <= cb, this chunk's loads came first
        const int s = n2 + lanes_below(m, lane);
        cand[s] = gi;
        keep[s] = sc;
        cq[s] = s2_hit_pos(off, ql, gi);
        croot[s] = hits[gi].root;
        if constexpr (kKind == 3) {
          cq[s] = nq - 1 - cq[s];
          croot[s] = croot[s] == 0 ? 0 : (int)(mirror - (uint32_t)croot[s]);
        }
        slots[s] = s;
      }
      n2 += __popcll(m);
    }
    ncand = n2;
  } else {
    ncand = 0;
  }
  wave_sync();
  // get_cells_fwd: by (root asc, score desc, querypos desc, hit asc); each root's best cells are the
  // first of its group and those with the same score
  wave_sort(lane, ncand, slots, sorted, sbuf, [&](int a, int b) {
    if (croot[a] != croot[b]) return croot[a] < croot[b];
    if (keep[a] != keep[b]) return keep[a] > keep[b];
    if (cq[a] != cq[b]) return cq[a] > cq[b];
    return kKind == 3 ? cand[a] > cand[b] : cand[a] < cand[b];  // (kind 3: the real hit order is the reverse)
  });
  int nkeep = 0, gcarry = 0;
  for (int cb = 0; cb < ncand; cb += 64) {
    const int i = cb + lane;
    int s = 0, gstart = 0;
    if (i < ncand) {
      s = sorted[i];
      gstart = (i == 0 || croot[sorted[i - 1]] != croot[s]) ? i : 0;
    }
    int m = gstart;  // the group's first element: running maximum of the group starts
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(m, o, 64);
      if (lane >= o) m = max(m, y);
    }
    m = max(m, gcarry);
    gcarry = __shfl(m, 63, 64);
    const bool k = i < ncand && keep[s] == keep[sorted[m]];
    const uint64_t bm = ballot(k);
    if (k) slots[nkeep + lanes_below(bm, lane)] = s;  // (slots is read no more)
    nkeep += __popcll(bm);
  }
  wave_sync();
  // Cell_score_cmp, stable over that order: (score desc, root asc, querypos desc, hit asc)
  wave_sort(lane, nkeep, slots, sorted, sbuf, [&](int a, int b) {
    if (keep[a] != keep[b]) return keep[a] > keep[b];
    if (croot[a] != croot[b]) return croot[a] < croot[b];
    if (cq[a] != cq[b]) return cq[a] > cq[b];
    return kKind == 3 ? cand[a] > cand[b] : cand[a] < cand[b];  // (kind 3: the real hit order is the reverse)
  });
  for (int i = lane; i < nkeep; i += 64) slots[i] = cand[sorted[i]];
  wave_sync();
  for (int i = lane; i < nkeep; i += 64) cand[i] = slots[i];
  wave_sync();
  int npaths = 0;
  constexpr int kMaxNalignments = kKind ? 1 : kS2MaxNalignments;  // (stage3.c:11382 / 15855 pass 1)
  while (npaths < nkeep && (npaths < kMaxNalignments || scs[cand[npaths]] == best)) npaths++;
  R.npaths = npaths;
  if constexpr (kKind == 1) {  // List_head(all_paths): paths are pushed, so the last cell the loop traced
    if (npaths > 1) {
      const int lastc = cand[npaths - 1];
      wave_sync();
      if (lane == 0) cand[0] = lastc;
      wave_sync();
      npaths = 1;
    }
  }

  S2_MARK(5);
  // ---- traceback_one per selected cell: length and extent of the converted list ----
  // the links go to LDS first (coalesced loads), so the pointer chases run at LDS latency
  // (past 4 096 hits the walk reads the hit arrays themselves: s2_walk_diag)
  extern __shared__ uint32_t s2c_lds[];
  uint32_t* llq = s2c_lds;
  uint32_t* lmap = s2c_lds + kS2cCap;
  const bool lds_walk = kLdsWalk;  // s2c_lds_class (checked above): 15-bit hit index, 16-bit querypos
  if (lds_walk && npaths > 0) {
    // 64 query positions per step (lane j holds off[cb + j]), their hits 64 at a time: a hit's position is
    // the last lane whose offset is <= the hit, a binary search over the lanes as in s2a_kernel's layout
    const S2Hit* __restrict__ hr = hits;
    const uint32_t* __restrict__ mr = maps;
    const int* __restrict__ offr = off;
    for (int cb = 0; cb < ql; cb += 64) {
      const int o = offr[min(cb + lane, ql)];
      const int hbeg = __shfl(o, 0, 64), hend = s2_u(offr[min(cb + 64, ql)]);
      for (int base = hbeg; base < hend; base += 64) {
        const int h = base + lane;
        int j = 0;
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) {
          const int oj = __shfl(o, j + st, 64);
          if (oj <= h) j += st;
        }
        if (h < hend) {
          const S2Hit x = hr[h];
          const uint32_t pr = x.pred >= 0 ? (uint32_t)x.pred : kS2NoPred;
          llq[h] = ((uint32_t)(cb + j) << 16) | (x.consec < kS2MinTerminal ? 0x8000u : 0u) | pr;
          lmap[h] = mr[h];
        }
      }
    }
  }
  wave_sync();
#ifdef GMAPDP_OI_TIMING
  if (threadIdx.x == 0) {
    atomicAdd(&g_s2_marks[1][13], (unsigned long long)npaths);
    atomicAdd(&g_s2_marks[1][14], (unsigned long long)wall_clock64());  // minus mark 5's time: the link table
  }
#endif
  // a single selected cell is the single result (Stage2_filter_unique keeps it): its walk records the
  // entries convert_to_nucleotides needs, and the second walk below is skipped
  const bool single = npaths == 1;
  // kind 3: a walk's n entries (mirrored, the cell's first) to the real call's, 3'-most hit first; lane e takes the
  // entries e and n - 1 - e
  auto unmirror = [&](int n) {
    wave_sync();
    for (int e = lane; 2 * e < n; e += 64) {
      const int f = n - 1 - e;
      const int qa = pathq[e], ha = pathh[e], qb = pathq[f], hb = pathh[f];
      pathq[e] = nq - 1 - qb;
      pathh[e] = (int)(mirror - (uint32_t)hb);
      pathq[f] = nq - 1 - qa;
      pathh[f] = (int)(mirror - (uint32_t)ha);
    }
    wave_sync();
  };
  (void)unmirror;
  for (int p = 0; p < npaths; p++) {
    const int cell = s2_u(cand[p]);
    int n = 0, top = -1, bottom = -1;
    if (lds_walk || nq <= 65536) {
      const S2WalkOut o = lds_walk ? s2_walk_wave(llq, lmap, cell, lane, single ? pathq : nullptr, pathh)
                                   : s2_walk_diag(hits, maps, scs, off, ql, cell, lane, single ? pathq : nullptr, pathh);
      n = o.n;
      top = o.top;
      bottom = o.bottom;
    } else if (lane == 0) {
      s2_walk(hits, maps, off, ql, cell, [&](int gi, int q) {
        if (n == 0) top = gi;
        bottom = gi;
        if (single) {
          pathq[n] = q;
          pathh[n] = (int)maps[gi];
        }
        n++;
      });
    }
    if constexpr (kKind == 3) {
      if (single) unmirror(s2_u(n));
    }
    if (lane == 0) {
      S2Path r;
      r.cell = cell;
      r.n = n;
      r.start = n ? (lds_walk ? lmap[bottom] : maps[bottom]) : 0u;
      r.end = n ? (lds_walk ? lmap[top] : maps[top]) + (uint32_t)(kS2K - 1) : 0u;
      if constexpr (kKind == 3) {  // the walk's first node is the real call's 5'-most, its last the 3'-most
        r.start = n ? mirror - (lds_walk ? lmap[top] : maps[top]) : 0u;
        r.end = n ? mirror - (lds_walk ? lmap[bottom] : maps[bottom]) + (uint32_t)(kS2K - 1) : 0u;
      }
      pth[p] = r;
    }
  }
  wave_sync();

  // ---- Stage2_filter_unique: stable sort by (start, end), drop each path overlapping an earlier one ----
  // (a path without entries has start = end = 0; it is no list, and below it neither counts as eliminated nor is kept)
  int* pord = cand;  // the selected cells live on in pth[].cell
  for (int i = lane; i < npaths; i += 64) keep[i] = i;
  wave_sync();
  wave_sort(lane, npaths, keep, pord, sbuf, [&](int a, int b) {
    if constexpr (kKind == 3) {  // stage2pairs_start_cmp (:5773): chrend descending, then chrstart descending
      if (pth[a].end != pth[b].end) return pth[a].end > pth[b].end;
      return pth[a].start > pth[b].start;
    }
    if (pth[a].start != pth[b].start) return pth[a].start < pth[b].start;
    return pth[a].end < pth[b].end;
  });
  for (int i = lane; i < npaths; i += 64) keep[i] = 0;  // eliminate flags, sorted order
  wave_sync();
  for (int i = 0; i < npaths; i++) {
    const S2Path x = pth[pord[i]];
    for (int j = i + 1 + lane; j < npaths; j += 64) {
      const S2Path y = pth[pord[j]];
      bool ov;
      if (y.start > x.end || x.start > y.end) {
        ov = false;
      } else if ((y.start < x.start && y.end >= x.end) || (y.start >= x.start && y.end < x.end)) {
        ov = true;  // subsumption
      } else {
        const uint32_t overlap = (y.start < x.start) ? y.end - x.start : x.end - y.start;
        const double fraction = (y.end - y.start < x.end - x.start) ? (double)overlap / (double)(y.end - y.start)
                                                                    : (double)overlap / (double)(x.end - x.start);
        ov = fraction > 0.5;
      }
      if (ov) keep[j] = 1;
    }
    wave_sync();
  }
  if constexpr (kKind != 0) {
    // a path without pairs is no list (Stage2_compute_one's NULL middle, _ends' `pairs != NULL`, _starts' `path !=
    // NULL`); ENDS / STARTS: when no list was eliminated only array[0] is kept (:6281-6283 / :6177-6179)
    int any = 0, first = -1;
    for (int i = 0; i < npaths; i++) {
      if (pth[pord[i]].n == 0) continue;
      if (first < 0) first = i;
      any |= keep[i];
    }
    wave_sync();
    for (int i = lane; i < npaths; i += 64)
      if (pth[pord[i]].n == 0 || (kKind >= 2 && !any && i != first)) keep[i] = 1;
    wave_sync();
  }
  int nres = 0;
  for (int i = 0; i < npaths; i++) nres += keep[i] ? 0 : 1;
  R.nresults = nres;

  S2_MARK(6);
  // ---- outputs: the kept results' path records and their pairs (convert_to_nucleotides) ----
  unsigned long long pbase = 0;
  if (lane == 0 && nres > 0) pbase = atomicAdd(&counters[1], (unsigned long long)nres);
  pbase = __shfl(pbase, 0, 64);
  if (nres > 0 && pbase + nres > path_cap) {
    if (lane == 0) {
      // (the reserved slots below the capacity become empty records: the pool's readers -- the fetch, pc_kernel --
      // count them, and would else see uninitialised memory or an earlier run's lists)
      for (unsigned long long k = pbase; k < path_cap; k++) paths_out[k] = gmapdp_path{0, 0, 0};
      R.status = kS2Overflow;
      results[P.index] = R;
    }
    return;
  }
  R.path_offset = (int32_t)pbase;
  const bool plusp = P.plusp != 0;
  const char* qs = qseq + P.qoff;
  const char* qu = quc + P.qoff;
  int r = 0, allpairs = 0;
  for (int i = 0; i < npaths; i++) {
    if (keep[i]) continue;
    const S2Path x = pth[pord[i]];
    const int n = x.n;
    if (!single && (lds_walk || nq <= 65536)) {  // entries, 3' end first
      if (lds_walk) (void)s2_walk_wave(llq, lmap, x.cell, lane, pathq, pathh);
      else (void)s2_walk_diag(hits, maps, scs, off, ql, x.cell, lane, pathq, pathh);
    } else if (lane == 0 && !single) {
      int e = 0;
      {
        s2_walk(hits, maps, off, ql, x.cell, [&](int gi, int q) {
          pathq[e] = q;
          pathh[e] = (int)maps[gi];
          e++;
        });
      }
    }
    wave_sync();
    if constexpr (kKind == 3) {
      if (!single) unmirror(n);
    }
    // records per entry in generation (prepend) order: [gap holder], fills, the observed pair.
    // Four 64-entry chunks per step, their loads issued together (the entries are in L2 scratch).
    constexpr int kC = 4;
    int total = 0;
    for (int cb = 0; cb < n; cb += 64 * kC) {
      int qp[kC], gp[kC], lqv[kC], lgv[kC];
#pragma unroll
      for (int k = 0; k < kC; k++) {
        const int e = cb + 64 * k + lane;
        qp[k] = e < n ? pathq[e] : 0;
        gp[k] = e < n ? pathh[e] : 0;
        lqv[k] = (e < n && e > 0) ? pathq[e - 1] : 0;
        lgv[k] = (e < n && e > 0) ? pathh[e - 1] : 0;
      }
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < kC; k++) {
        const int e = cb + 64 * k + lane;
        if (e < n) {
          int fill, gap;
          s2_entry_v(e, qp[k], gp[k], lqv[k], lgv[k], fill, gap);
          if constexpr (kKind >= 2) gap = 0;  // include_gapholders_p false
          cnt += gap + fill + 1;
        }
      }
      total += wave_sum_i(cnt);
    }
    unsigned long long qb = 0;
    if (lane == 0) qb = atomicAdd(&counters[2], (unsigned long long)total);
    qb = __shfl(qb, 0, 64);
    if (qb + total > pair_cap) {
      if (lane == 0) {
        // (the lists written so far stay; the call's other reserved path slots become empty records, as above)
        for (int k = r; k < nres; k++) paths_out[pbase + k] = gmapdp_path{0, 0, 0};
        R.status = kS2Overflow;
        results[P.index] = R;
      }
      return;
    }
    gmapdp_path_pair* dst = pairs_out + qb;
    // record of generation index g (the order convert_to_nucleotides pushes: 3' end first): the list runs 5' end
    // first; Stage2_compute_one returns it reversed
    auto slot = [&](int g) { return (kKind == 1 || kKind == 3) ? g : total - 1 - g; };
    const int qoffs = kKind ? P.query_offset : 0;
    int gen = 0;
    for (int cb = 0; cb < n; cb += 64 * kC) {
      int qp[kC], gp[kC], lqv[kC], lgv[kC];
#pragma unroll
      for (int k = 0; k < kC; k++) {
        const int e = cb + 64 * k + lane;
        qp[k] = e < n ? pathq[e] : 0;
        gp[k] = e < n ? pathh[e] : 0;
        lqv[k] = (e < n && e > 0) ? pathq[e - 1] : 0;
        lgv[k] = (e < n && e > 0) ? pathh[e - 1] : 0;
      }
      char cq[kC], cu[kC];
#pragma unroll
      for (int k = 0; k < kC; k++) {
        const int e = cb + 64 * k + lane;
        cq[k] = e < n ? qs[qp[k]] : 0;
        cu[k] = e < n ? qu[qp[k]] : 0;
      }
#pragma unroll
      for (int k = 0; k < kC; k++) {
        const int e = cb + 64 * k + lane;
        int cnt = 0, fill = 0, gap = 0;
        if (e < n) {
          s2_entry_v(e, qp[k], gp[k], lqv[k], lgv[k], fill, gap);
          if constexpr (kKind >= 2) gap = 0;
          cnt = gap + fill + 1;
        }
        const int incl = wave_incl_sum(cnt, lane);
        if (e < n) {
          int g = gen + incl - cnt;  // generation index of the entry's first record
          const int qpos = qp[k], gpos = gp[k];
          if (gap) {
            gmapdp_path_pair rr;
            rr.querypos = rr.genomepos = -1;
            rr.queryjump = (lqv[k] - 1 - qpos) - fill;
            rr.genomejump = (lgv[k] - 1 - gpos) - fill;
            rr.cdna = rr.comp = rr.genome = rr.genomealt = ' ';
            dst[slot(g++)] = rr;
          }
          for (int j = 0; j < fill; j++) {
            const int lq = qpos + fill - j, lg = gpos + fill - j;
            const char c = s2_genomic_nt(blocks, nwords, (uint32_t)lg, P.chroffset, P.chrhigh, plusp);
            gmapdp_path_pair rr;
            rr.querypos = lq + qoffs;
            rr.genomepos = lg;
            rr.queryjump = rr.genomejump = 0;
            rr.cdna = qs[lq];
            rr.comp = '|';
            if constexpr (kModal) rr.comp = qu[lq] == c ? '|' : ':';  // queryuc against the genome (:5405)
            rr.genome = rr.genomealt = c;
            dst[slot(g++)] = rr;
          }
          gmapdp_path_pair rr;
          rr.querypos = qpos + qoffs;
          rr.genomepos = gpos;
          rr.queryjump = rr.genomejump = 0;
          rr.cdna = cq[k];
          rr.comp = '|';
          rr.genome = rr.genomealt = cu[k];
          if constexpr (kModal) {
            // the observed pair is kept only when its cdna -- the query as given, compared case-sensitively --
            // equals the genome's character, else re-pushed with ':' (:5434-5451); kept, its genome is queryuc,
            // which then equals that character
            const char c = s2_genomic_nt(blocks, nwords, (uint32_t)gpos, P.chroffset, P.chrhigh, plusp);
            rr.comp = cq[k] == c ? '|' : ':';
            rr.genome = rr.genomealt = c;
          }
          dst[slot(g)] = rr;
        }
        gen += __shfl(incl, 63, 64);
      }
    }
    if (lane == 0) {
      gmapdp_path pr;
      pr.pair_offset = (int64_t)qb;
      pr.npairs = total;
      pr.pad_ = 0;
      paths_out[pbase + r] = pr;
    }
    r++;
    allpairs += total;
    wave_sync();
  }
  R.npairs = allpairs;
  if (lane == 0) results[P.index] = R;
  S2_MARK(7);
}

#ifdef GMAPDP_OI_TIMING
extern "C" int gmapdp_debug_s2_sub(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_s2_sub), sizeof(g_s2_sub)) != hipSuccess) return 1;
  static const unsigned long long zero[2][8] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_s2_sub), zero, sizeof(zero)) != hipSuccess;
}
extern "C" int gmapdp_debug_s2_waves(unsigned int* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_s2_wave), sizeof(g_s2_wave)) != hipSuccess;
}
extern "C" int gmapdp_debug_s2_marks(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_s2_marks), sizeof(g_s2_marks)) != hipSuccess) return 1;
  static const unsigned long long zero[2][16] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_s2_marks), zero, sizeof(zero)) != hipSuccess;
}
#endif

// the canonical sweeps' counters (g_s2_canon) since the last call, then cleared; the device must be idle
int s2_canon_counters(unsigned long long* out8) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_s2_canon), sizeof(g_s2_canon)) != hipSuccess) return 1;
  static const unsigned long long zero[8] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_s2_canon), zero, sizeof(zero)) != hipSuccess;
}

size_t scratch_bytes_s2c(int querylength, int totalpositions, int ndiagonals) {
  return s2_scratch(querylength, totalpositions, ndiagonals).total;
}

hipError_t launch_s2c(int nproblems, hipStream_t stream, const DevStage2Problem* probs, const uint32_t* blocks,
                      uint64_t nwords, const char* qseq, const char* quc, const gmapdp_oligo_result* ores,
                      const int32_t* npos, const int32_t* map, const uint32_t* table, const int32_t* diags,
                      unsigned char* scratch, unsigned long long* counters, unsigned long long scratch_cap,
                      gmapdp_stage2_result* results, gmapdp_path* paths, unsigned long long path_cap,
                      gmapdp_path_pair* pairs, unsigned long long pair_cap, bool modal, int phases,
                      const double* canon_metab, int kind) {
  // kind: the batch's DevStage2Problem.kind (0 Stage2_compute, GMAPDP_S2X_ONE / _ENDS / _STARTS): the sweep's and
  // the path kernels' variant; STARTS also the layout's (s2a_starts_kernel)
  // canon_metab: the MaxEnt tables of a GMAPDP_S2_CANONICAL_MIDDLE batch (the sweep's canonical variant), else NULL
  void* args[] = {(void*)&probs, (void*)&blocks, (void*)&nwords, (void*)&qseq, (void*)&quc, (void*)&ores,
                  (void*)&npos, (void*)&map, (void*)&table, (void*)&diags, (void*)&scratch, (void*)&counters,
                  (void*)&scratch_cap, (void*)&results, (void*)&paths, (void*)&path_cap, (void*)&pairs,
                  (void*)&pair_cap, (void*)&canon_metab};
  // phases (bits): 1 the order + s2a, 2 s2b, 4 s2c; one phase alone re-runs it over the previous run's
  // scratch (the bench's per-kernel timing)
  hipError_t e = hipSuccess;
  if (phases & 1) {
    const int* nowork = nullptr;
    void* oargs0[] = {(void*)&probs, (void*)&nproblems, (void*)&ores, (void*)&counters, (void*)&nowork};
    e = hipLaunchKernel(reinterpret_cast<void*>(&s2_order_kernel), dim3(1), dim3(kS2OrderThreads), oargs0, 0, stream);
    if (e == hipSuccess)
      e = hipLaunchKernel(kind == 3 ? reinterpret_cast<void*>(&s2a_starts_kernel) : reinterpret_cast<void*>(&s2a_kernel),
                          dim3(nproblems), dim3(64), args, 0, stream);
    // the sweep (and s2c) heaviest first by s2a's work estimate
    const int* work = reinterpret_cast<const int*>(counters + 4) + nproblems;
    void* oargs1[] = {(void*)&probs, (void*)&nproblems, (void*)&ores, (void*)&counters, (void*)&work};
    if (e == hipSuccess)
      e = hipLaunchKernel(reinterpret_cast<void*>(&s2_order_kernel), dim3(1), dim3(kS2OrderThreads), oargs1, 0,
                          stream);
  }
  if (e == hipSuccess && (phases & 2)) {
    // GMAPDP_S2B_LDS (experiments): extra LDS per sweep wave, to cap its waves per CU
    static const size_t xlds = [] {
      const char* v = std::getenv("GMAPDP_S2B_LDS");
      return v ? (size_t)std::strtoull(v, nullptr, 10) : (size_t)0;
    }();
    void* sweep = kind == 1   ? reinterpret_cast<void*>(&s2b_one_kernel)
                  : kind == 2 ? reinterpret_cast<void*>(&s2b_ends_kernel)
                  : kind == 3 ? reinterpret_cast<void*>(&s2b_starts_kernel)
                  : canon_metab ? reinterpret_cast<void*>(&s2b_canon_kernel)
                                : reinterpret_cast<void*>(&s2b_kernel);
    if (xlds > 64 * 1024) e = hipFuncSetAttribute(sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)xlds);
    if (e == hipSuccess) e = hipLaunchKernel(sweep, dim3(nproblems), dim3(64), args, xlds, stream);
  }
  if (e == hipSuccess && (phases & 4)) {  // the heavy calls (first in the order) without LDS, then the rest
    // (modal: a cmet / atoi / ttoc context's pair emission, convert_to_nucleotides outside STANDARD)
    void* heavy = modal ? reinterpret_cast<void*>(&s2c_kernel<false, true>)
                        : reinterpret_cast<void*>(&s2c_kernel<false, false>);
    void* rest = modal ? reinterpret_cast<void*>(&s2c_kernel<true, true>)
                       : reinterpret_cast<void*>(&s2c_kernel<true, false>);
    if (kind == 1) {
      heavy = modal ? reinterpret_cast<void*>(&s2c_kernel<false, true, 1>)
                    : reinterpret_cast<void*>(&s2c_kernel<false, false, 1>);
      rest = modal ? reinterpret_cast<void*>(&s2c_kernel<true, true, 1>)
                   : reinterpret_cast<void*>(&s2c_kernel<true, false, 1>);
    } else if (kind == 2) {
      heavy = modal ? reinterpret_cast<void*>(&s2c_kernel<false, true, 2>)
                    : reinterpret_cast<void*>(&s2c_kernel<false, false, 2>);
      rest = modal ? reinterpret_cast<void*>(&s2c_kernel<true, true, 2>)
                   : reinterpret_cast<void*>(&s2c_kernel<true, false, 2>);
    } else if (kind == 3) {
      heavy = modal ? reinterpret_cast<void*>(&s2c_kernel<false, true, 3>)
                    : reinterpret_cast<void*>(&s2c_kernel<false, false, 3>);
      rest = modal ? reinterpret_cast<void*>(&s2c_kernel<true, true, 3>)
                   : reinterpret_cast<void*>(&s2c_kernel<true, false, 3>);
    }
    e = hipLaunchKernel(heavy, dim3(nproblems), dim3(64), args, 0, stream);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(rest, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(8 * kS2cCap));
    if (e == hipSuccess) e = hipLaunchKernel(rest, dim3(nproblems), dim3(64), args, 8 * kS2cCap, stream);
  }
  return e;
}

}  // namespace gmapdp
