/* tests/s2soracle/s2s_oracle.c -- TEST INFRASTRUCTURE ONLY (never shipped, never on the product path).
 *
 * CPU restatement of the stage-2 entry point stage 3 calls on an unaligned 5' end (paths under the reference
 * tree's src/):
 *
 *   Stage2_compute_starts  stage2.c:6914, as stage3.c:15955 / 16166 call it (localp false, skip_repetitive_p
 *                          false, favor_right_p false, max_nalignments 1; middlep false inside)
 *
 * with use_canonical_middle_p false, genomealt == genome, genestrand 0, mode STANDARD, no SNPs.  The seeding
 * (the minor oligoindex) and the genome come from oracle/libgmapdp_oracle.so.  The chain is
 * align_compute_lookforward (:5062), restated here directly, function by function, in the direction the
 * reference runs it -- nothing is mirrored and no lookback function is called, so that this oracle can check an
 * engine that does mirror:
 *
 *   the sweep                  align_compute_scores_lookforward (:4610): from the last query position down; the
 *                              processed list holds positions further 3'; the hit loops and the active chains
 *                              run from high_hit - 1 down (revise_active_lookforward :3034), so the best hit of
 *                              a position on a tie is the highest
 *   score_one / score_mult     score_querypos_lookforward_one / _mult (:2020 / :2404): querydistance =
 *                              prev_querypos - curr_querypos, a previous hit is adjacent at position +
 *                              querydistance, ranges 1-4 compare prevposition against position + ... from above
 *   localp / middlep false     as in Stage2_compute_ends: a hit without a predecessor keeps score 0 (fwd_tracei
 *                              advances; not in _mult's last_item == NULL branch), a position none of whose
 *                              hits scored above 0 restarts every hit at score 8 (:4895-4920)
 *   the grand lookforward      :4923-4950, valid while grand_fwd_querypos <= querylength - indexsize
 *   get_cells_fwd              :3437, the function the lookback uses, on real coordinates
 *   traceback_one              :4140: from the cell along fwd_pos / fwd_hit, i.e. towards the 3' end; the
 *                              MIN_TERMINAL_NCONSECUTIVE pruning eats the path's 5' end; the pushed list's head is
 *                              the 3'-most hit
 *   convert_to_nucleotides     :5334 without gap holders; List_reverse(pairs): each list 3' end first
 *   the filter                 Stage2pairs_filter_unique_starts (:6114): stable sort by stage2pairs_start_cmp
 *                              (:5773: the first pair's genomepos descending, then the last pair's descending),
 *                              every list overlapping an earlier one eliminated (stage2path_overlap_p :5837);
 *                              nothing eliminated: only array[0] is kept
 *
 * glibc's qsort is a stable merge sort for these sizes, so is stable_sort below.  Per call the rules above are
 * counted (S2S_* below).  Pinned against the reference's own function by tests/test_stage2_starts_oracle.py over
 * tests/golden/stage2_starts_golden.npz.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "gmapdp_oracle.h"

#define INDEXSIZE 8
#define EQUAL_DISTANCE_NOT_SPLICING 9
#define ENOUGH_CONSECUTIVE 32
#define GREEDY_NCONSECUTIVE 100
#define EXON_DEFN 30
#define MIN_TERMINAL_NCONSECUTIVE 8
#define MAX_NACTIVE 100
#define SCORE_FOR_RESTRICT 10
#define TEN_THOUSAND 8192
#define FINAL_SCORE_TOLERANCE 20
#define MAX_NALIGNMENTS 1
#define SUFFLOOKBACK 60
#define NSUFFLOOKBACK 5

/* counters (per call, added to the caller's array) */
enum { S2S_RESTART, S2S_ZERO_EARLY, S2S_BIG_POSITION, S2S_TIED_CELLS, S2S_ELIMINATED, S2S_FIRST_KEPT, S2S_PRUNED,
       S2S_NCOUNTERS };

static void
stable_sort (void **a, int n, int (*cmp) (const void *, const void *)) {
  void **tmp;
  int width, i, l, m, r, x, y, k;
  if (n < 2) return;
  tmp = (void **) malloc((size_t) n * sizeof(void *));
  for (width = 1; width < n; width *= 2) {
    for (i = 0; i < n; i += 2 * width) {
      l = i; m = i + width < n ? i + width : n; r = i + 2 * width < n ? i + 2 * width : n;
      x = l; y = m; k = l;
      while (x < m && y < r) tmp[k++] = (cmp(&a[y], &a[x]) < 0) ? a[y++] : a[x++];
      while (x < m) tmp[k++] = a[x++];
      while (y < r) tmp[k++] = a[y++];
    }
    memcpy(a, tmp, (size_t) n * sizeof(void *));
  }
  free(tmp);
}

typedef struct {
  const unsigned int *map;
  const int *npos, *off;
  int *consec, *root, *fpos, *fhit, *tracei, *score, *active, *firstactive;
  int tracectr, splicingp;
  unsigned int maxintronlen;
  long *cnt;
} Chain;

#define MAP(C, q, h) ((C)->map[(C)->off[q] + (h)])
#define LNK(C, f, q, h) ((C)->f[(C)->off[q] + (h)])

typedef struct {
  int consec, root, pp, ph, score, tracei;
} Best;

/* the tail of score_querypos_lookforward_one (:2368-2387) and of _mult's general branch (:2915-2935), localp false */
static void
finish_link (Chain *C, int q, int hit, const Best *b) {
  int gi = C->off[q] + hit;
  C->consec[gi] = b->consec;
  C->root[gi] = b->root;
  C->fpos[gi] = b->pp;
  C->fhit[gi] = b->ph;
  if (b->pp >= 0) {
    C->tracei[gi] = b->tracei;
    C->score[gi] = b->score;
  } else {
    C->tracei[gi] = ++C->tracectr;
    C->score[gi] = b->score;   /* as the search left it: 0 */
  }
}

/* section D for one previous position pq (> q) from its active hit ph on: ranges 0-4 (:2157-2360, :2714-2905).
   The active chain descends in chrpos.  Returns the hit after range 1 (_mult's frontier). */
static int
score_ranges (Chain *C, Best *b, int q, unsigned int position, int pq, int ph, int *last_tr, int range1) {
  int qd = pq - q, credit = -qd / INDEXSIZE, gendist, diff, fs, frontier;
  unsigned int pp;
  while (ph != -1 && LNK(C, tracei, pq, ph) == *last_tr) ph = LNK(C, active, pq, ph);   /* range 0 */
  if (ph != -1) *last_tr = LNK(C, tracei, pq, ph);
  if (range1)
    while (ph != -1 && MAP(C, pq, ph) >= position + C->maxintronlen + (unsigned int) qd) ph = LNK(C, active, pq, ph);
  frontier = ph;
  while (ph != -1 && (pp = MAP(C, pq, ph)) > position + EQUAL_DISTANCE_NOT_SPLICING + (unsigned int) qd) {  /* range 2 */
    gendist = (int) (pp - position);
    diff = gendist - qd;
    fs = LNK(C, score, pq, ph) + credit - (C->splicingp ? (diff / TEN_THOUSAND + 1) : (diff + 1));
    if (fs > b->score) {
      b->consec = (diff <= 0) ? LNK(C, consec, pq, ph) + qd : 0;
      b->root = LNK(C, root, pq, ph);
      b->score = fs;
      b->pp = pq;
      b->ph = ph;
      b->tracei = ++C->tracectr;
    }
    ph = LNK(C, active, pq, ph);
  }
  while (ph != -1 && (pp = MAP(C, pq, ph)) >= position + INDEXSIZE) {   /* ranges 3-4 */
    gendist = (int) (pp - position);
    diff = gendist > qd ? gendist - qd : qd - gendist;
    fs = LNK(C, score, pq, ph) + 1;
    if (fs > b->score) {
      b->consec = (diff <= 0) ? LNK(C, consec, pq, ph) + qd : 0;
      b->root = LNK(C, root, pq, ph);
      b->score = fs;
      b->pp = pq;
      b->ph = ph;
      b->tracei = LNK(C, tracei, pq, ph);
    }
    ph = LNK(C, active, pq, ph);
  }
  return frontier;
}

/* section A's search (:2082-2087): down the active chain of pq while its hit lies above position + qd */
static int
adjacent (Chain *C, int pq, int *ph_io, int qd, unsigned int position) {
  int ph = *ph_io;
  unsigned int pp = position;
  while (ph != -1 && (pp = MAP(C, pq, ph)) > position + (unsigned int) qd) ph = LNK(C, active, pq, ph);
  *ph_io = ph;
  return pp == position + (unsigned int) qd;
}

/* score_querypos_lookforward_one (stage2.c:2020); proc[0..np) oldest first (proc[np - 1] = Intlist_head) */
static void
score_one (Chain *C, int q, int hit, const int *proc, int np) {
  unsigned int position = MAP(C, q, hit);
  Best b = {INDEXSIZE, (int) position, -1, -1, 0, 0};
  int nlookback = NSUFFLOOKBACK, lookback = SUFFLOOKBACK, k, nseen, donep, last_tr, pq, qd, ph;
  if (np > 0) {
    pq = proc[np - 1];
    qd = pq - q;
    ph = C->firstactive[pq];
    if (adjacent(C, pq, &ph, qd, position)) {
      b.consec = LNK(C, consec, pq, ph) + qd;
      b.root = LNK(C, root, pq, ph);
      b.score = LNK(C, score, pq, ph) + qd;
      b.pp = pq;
      b.ph = ph;
      b.tracei = LNK(C, tracei, pq, ph);
      nlookback = 1;
      lookback = SUFFLOOKBACK / 2;
    }
  }
  donep = 0;
  last_tr = -1;
  for (k = np - 1, nseen = 0; k >= 0 && b.consec < ENOUGH_CONSECUTIVE && !donep; k--, nseen++) {
    pq = proc[k];
    qd = pq - q;
    if (nseen > nlookback && qd - INDEXSIZE > lookback) donep = 1;
    if ((ph = C->firstactive[pq]) != -1) score_ranges(C, &b, q, position, pq, ph, &last_tr, C->splicingp);
  }
  finish_link(C, q, hit, &b);
}

/* score_querypos_lookforward_mult (stage2.c:2404) over hits [low, high), the highest first */
static void
score_mult (Chain *C, int q, int low, int high, const int *proc, int np) {
  int nhits = high - low, hiti, adj, adq, n, maxadj = 0, maxnon = 0, overall = 0, adjf, ph, maxseen, nseen, k,
      last_tr, pq, qd;
  int *frontier;
  unsigned int position;
  Best b;
  if (np == 0) {   /* last_item == NULL (:2468-2489) */
    for (hiti = nhits - 1; hiti >= 0; hiti--) {
      int gi = C->off[q] + low + hiti;
      C->consec[gi] = INDEXSIZE;
      C->root[gi] = (int) MAP(C, q, low + hiti);
      C->fpos[gi] = C->fhit[gi] = -1;
      C->score[gi] = 0;   /* localp false; fwd_tracei keeps what it held */
      C->cnt[S2S_ZERO_EARLY]++;
    }
    return;
  }
  /* (the branch processed == NULL with last_item != NULL, :2491, needs MOVE_TO_STAGE3) */
  adj = proc[np - 1];
  adq = adj - q;
  frontier = (int *) malloc((size_t) np * sizeof(int));
  for (n = 0; n < np; n++) {
    qd = proc[np - 1 - n] - q;
    if (n <= 1 || qd - INDEXSIZE <= SUFFLOOKBACK / 2) maxadj = n;
    if (n <= NSUFFLOOKBACK || qd - INDEXSIZE <= SUFFLOOKBACK) maxnon = n;
    frontier[n] = C->firstactive[proc[np - 1 - n]];
  }
  adjf = C->firstactive[adj];
  for (hiti = nhits - 1; hiti >= 0; hiti--) {   /* overall_fwd_consecutive (:2617-2637) */
    position = MAP(C, q, low + hiti);
    ph = adjf;
    if (adjacent(C, adj, &ph, adq, position) && LNK(C, consec, adj, ph) + adq > overall)
      overall = LNK(C, consec, adj, ph) + adq;
    adjf = ph;
  }
  adjf = C->firstactive[adj];
  for (hiti = nhits - 1; hiti >= 0; hiti--) {
    position = MAP(C, q, low + hiti);
    ph = adjf;
    if (adjacent(C, adj, &ph, adq, position)) {
      b.consec = LNK(C, consec, adj, ph) + adq;
      b.root = LNK(C, root, adj, ph);
      b.pp = adj;
      b.ph = ph;
      b.score = LNK(C, score, adj, ph) + adq;
      b.tracei = LNK(C, tracei, adj, ph);
      maxseen = maxadj;
    } else {
      b.consec = INDEXSIZE;
      b.root = (int) position;
      b.pp = b.ph = -1;
      b.score = 0;
      b.tracei = -1;
      maxseen = maxnon;
    }
    adjf = ph;
    if (overall < GREEDY_NCONSECUTIVE) {
      last_tr = -1;
      for (k = np - 1, nseen = 0; k >= 0 && b.consec < ENOUGH_CONSECUTIVE && nseen <= maxseen; k--, nseen++) {
        if ((ph = frontier[nseen]) != -1) {
          pq = proc[k];
          frontier[nseen] = score_ranges(C, &b, q, position, pq, ph, &last_tr, 1);
        }
      }
    }
    finish_link(C, q, low + hiti, &b);
  }
  free(frontier);
}

/* revise_active_lookforward (stage2.c:3034): the active chain from the highest hit down */
static void
revise_active (Chain *C, int q, int low, int high) {
  int best, threshold, hit, *ptr;
  if (high - 1 < low) {
    C->firstactive[q] = -1;
    return;
  }
  best = LNK(C, score, q, high - 1);
  for (hit = high - 2; hit >= low; hit--)
    if (LNK(C, score, q, hit) > best) best = LNK(C, score, q, hit);
  threshold = best - SCORE_FOR_RESTRICT;
  if (threshold < 0) threshold = 0;
  C->firstactive[q] = -1;
  ptr = &C->firstactive[q];
  hit = high - 1;
  while (hit >= low) {
    while (hit >= low && LNK(C, score, q, hit) <= threshold) hit--;
    *ptr = hit;
    if (hit >= low) {
      ptr = &LNK(C, active, q, hit);
      hit--;
    }
  }
  *ptr = -1;
}

typedef struct {
  int root, endpos, querypos, hit, score;
} OCell;

static int
cell_root_cmp (const void *x, const void *y) {   /* Cell_rootposition_left_cmp (stage2.c:3230) */
  const OCell *a = *(OCell * const *) x, *b = *(OCell * const *) y;
  if (a->root != b->root) return a->root < b->root ? -1 : 1;
  if (a->score != b->score) return a->score > b->score ? -1 : 1;
  if (a->querypos != b->querypos) return a->querypos > b->querypos ? -1 : 1;
  if (a->hit != b->hit) return a->hit < b->hit ? -1 : 1;
  return 0;
}

static int
cell_score_cmp (const void *x, const void *y) {  /* Cell_score_cmp (stage2.c:3323) */
  const OCell *a = *(OCell * const *) x, *b = *(OCell * const *) y;
  return (a->score > b->score) ? -1 : (b->score > a->score) ? 1 : 0;
}

typedef struct {
  OrcPair *p;
  int n, cap, overflow;
} Sink;

static void
push (Sink *s, int querypos, int genomepos, char cdna, char comp, char g, char galt) {
  OrcPair *r;
  if (querypos < 0 || genomepos < 0) return;  /* Pairpool_push (pairpool.c:190) */
  if (s->n >= s->cap) { s->overflow = 1; return; }
  r = &s->p[s->n++];
  memset(r, 0, sizeof(*r));
  r->querypos = querypos;
  r->genomepos = genomepos;
  r->cdna = cdna;
  r->comp = comp;
  r->genome = g;
  r->genomealt = galt;
}

static const char complement_lc[128] =
  "???????????????????????????????? ??#$%&')(*+,-./0123456789:;>=<??TVGHEFCDIJMLKNOPQYSAABWXRZ]?[^_`tvghefcdijmlknopqysaabwxrz}|{~?";

/* get_genomic_nt (stage2.c:4124): no chromosome-bound check */
static char
genomic_nt (unsigned int chrpos, unsigned int chroffset, unsigned int chrhigh, int plusp) {
  unsigned int length;
  const char *g = orc_genome_seq(&length);
  unsigned int pos = plusp ? chroffset + chrpos : chrhigh - chrpos;
  char c = (pos < length) ? g[pos] : 'N';
  if (c != 'A' && c != 'C' && c != 'G' && c != 'T') c = 'N';
  if (!plusp) c = complement_lc[(int) c];
  return c;
}

/* traceback_one (stage2.c:4140) from cell (q, hit) forward + convert_to_nucleotides (:5334) without gap holders +
   List_reverse.  traceback_one pushes the hits as it walks towards the 3' end, so the path's head, which
   convert_to_nucleotides takes first, is the last hit walked.  The records are appended in the order
   convert_to_nucleotides pushes them, which is the reversed list's order: 3' end first.  Returns the number of
   records appended. */
static int
emit_path (Chain *C, Sink *s, int q, int hit, const char *queryseq, const char *queryuc, int query_offset,
           unsigned int chroffset, unsigned int chrhigh, int plusp, int *pathq, int *pathh) {
  int n = 0, pq, i, start = s->n, lastq, lastg, qj, gj, fill, querypos, genomepos, pruned = 0;
  char c;
  while (q >= 0 && LNK(C, consec, q, hit) < MIN_TERMINAL_NCONSECUTIVE) {   /* prune the walk's start: the 5' end */
    pq = q;
    q = LNK(C, fpos, pq, hit);
    hit = LNK(C, fhit, pq, hit);
    pruned = 1;
  }
  if (pruned) C->cnt[S2S_PRUNED]++;
  while (q >= 0) {
    if ((int) MAP(C, q, hit) >= 0) { pathq[n] = q; pathh[n] = hit; n++; }
    pq = q;
    q = LNK(C, fpos, pq, hit);
    hit = LNK(C, fhit, pq, hit);
  }
  if (n == 0) return 0;
  querypos = pathq[n - 1];
  genomepos = (int) MAP(C, pathq[n - 1], pathh[n - 1]);
  for (lastq = querypos + INDEXSIZE - 1, lastg = genomepos + INDEXSIZE - 1; lastq > querypos; lastq--, lastg--) {
    c = genomic_nt((unsigned int) lastg, chroffset, chrhigh, plusp);
    push(s, lastq + query_offset, lastg, queryseq[lastq], '|', c, c);
  }
  push(s, querypos + query_offset, genomepos, queryseq[querypos], '|', queryuc[querypos], queryuc[querypos]);
  lastq = querypos;
  lastg = genomepos;
  for (i = n - 2; i >= 0; i--) {
    querypos = pathq[i];
    genomepos = (int) MAP(C, pathq[i], pathh[i]);
    qj = lastq - 1 - querypos;
    gj = lastg - 1 - genomepos;
    if (qj != 0 || gj != 0) {
      if (querypos + INDEXSIZE - 1 >= lastq || genomepos + INDEXSIZE - 1 >= lastg)
        fill = (lastq - querypos < lastg - genomepos) ? lastq - querypos - 1 : lastg - genomepos - 1;
      else
        fill = INDEXSIZE - 1;
      for (lastq = querypos + fill, lastg = genomepos + fill; lastq > querypos; lastq--, lastg--) {
        c = genomic_nt((unsigned int) lastg, chroffset, chrhigh, plusp);
        push(s, lastq + query_offset, lastg, queryseq[lastq], '|', c, c);
      }
    }
    push(s, querypos + query_offset, genomepos, queryseq[querypos], '|', queryuc[querypos], queryuc[querypos]);
    lastq = querypos;
    lastg = genomepos;
  }
  return s->n - start;
}

typedef struct {
  int offset, npairs;
  unsigned int start, end;    /* chrstart: the last pair's genomepos; chrend: the first pair's */
} OPath;

static int
path_cmp (const void *x, const void *y) {   /* stage2pairs_start_cmp (stage2.c:5773) */
  const OPath *a = *(OPath * const *) x, *b = *(OPath * const *) y;
  if (a->end != b->end) return a->end > b->end ? -1 : 1;
  if (a->start != b->start) return a->start > b->start ? -1 : 1;
  return 0;
}

/* stage2path_overlap_p (stage2.c:5837) */
static int
overlap_p (const OPath *x, const OPath *y) {
  unsigned int overlap;
  double fraction;
  if (y->start > x->end || x->start > y->end) return 0;
  if (y->start < x->start) {
    if (y->end < x->end) {
      overlap = y->end - x->start;
      fraction = (y->end - y->start < x->end - x->start) ? (double) overlap / (double) (y->end - y->start)
                                                         : (double) overlap / (double) (x->end - x->start);
      return fraction > 0.5;
    }
    return 1;
  }
  if (y->end < x->end) return 1;
  overlap = x->end - y->start;
  fraction = (y->end - y->start < x->end - x->start) ? (double) overlap / (double) (y->end - y->start)
                                                     : (double) overlap / (double) (x->end - x->start);
  return fraction > 0.5;
}

/* scalars[0..5] = {lists returned, paths traced, ncovered, status (0 no positions, 2 chained), querystart,
   queryend}; paths[2 k], paths[2 k + 1] = first record and record count of returned list k, in the returned
   list's order; counters[S2S_NCOUNTERS] (may be NULL) are added to.  Returns the number of lists, -1 when a
   capacity is too small, the seeding's error (< -1) otherwise. */
static int
stage2s (const char *queryseq, const char *queryuc, int querylength, int query_offset, unsigned int chrstart,
         unsigned int chrend, unsigned int chroffset, unsigned int chrhigh, int plusp, int splicingp,
         int maxintronlen, int *scalars, int *paths, int path_cap, OrcPair *pairs, int pair_cap, long *counters) {
  int *npos, sc[4], *dg, nd, T, i, q, hit, ncovered, count, *cover, qend, low, high, best_hit, best_score,
      grand_score, grand_q, grand_hit, *proc, np, ncells, k, bestscore, npaths, nkept = 0, *pathq, *pathh, rc;
  unsigned int *positions, chrinit, chrterm, position, prevposition;
  long nocount[S2S_NCOUNTERS];
  Chain Cst, *C = &Cst;
  OCell *cellv, **cells, **sorted;
  Sink sink = {pairs, 0, pair_cap, 0};
  int pos_cap = 1 << 22, diag_cap = 1 << 16;

  for (i = 0; i < 6; i++) scalars[i] = 0;
  npos = (int *) calloc((size_t) querylength + 1, sizeof(int));
  positions = (unsigned int *) malloc((size_t) pos_cap * sizeof(unsigned int));
  dg = (int *) malloc((size_t) diag_cap * 4 * sizeof(int));
  rc = orc_oligo_mappings(queryuc, querylength, chrstart, chrend, chroffset, chrhigh, plusp, /*minor*/1, npos,
                          positions, pos_cap, sc, dg, diag_cap);
  if (rc < 0) {
    free(npos); free(positions); free(dg);
    return rc;
  }
  T = sc[0];
  nd = sc[3];
  /* Diag_update_coverage (diag.c:216): computed, not tested */
  cover = (int *) calloc((size_t) querylength + 1, sizeof(int));
  for (i = 0; i < nd; i++) {
    cover[dg[4 * i + 1]] += 1;
    cover[dg[4 * i + 2]] -= 1;
  }
  for (q = 0, count = 0, ncovered = 0; q < querylength; q++) {
    count += cover[q];
    if (count > 0) ncovered++;
  }
  free(cover);
  free(dg);
  scalars[2] = ncovered;
  scalars[3] = T > 0 ? 2 : 0;
  if (T <= 0) {
    free(npos); free(positions);
    return 0;
  }
  /* Diag_max_bounds (diag.c:894) */
  chrinit = plusp ? chrstart : (chrhigh - chroffset) - chrend;
  chrterm = plusp ? chrend : (chrhigh - chroffset) - chrstart;
  qend = querylength - 1;
  scalars[4] = 0;
  scalars[5] = qend;

  memset(C, 0, sizeof(*C));
  memset(nocount, 0, sizeof(nocount));
  C->cnt = counters ? counters : nocount;
  C->npos = npos;
  C->map = positions;
  {
    int *off = (int *) malloc(((size_t) querylength + 1) * sizeof(int));
    for (q = 0, off[0] = 0; q < querylength; q++) off[q + 1] = off[q] + npos[q];
    C->off = off;
  }
  C->consec = (int *) calloc((size_t) T + 1, sizeof(int));
  C->root = (int *) calloc((size_t) T + 1, sizeof(int));
  C->fpos = (int *) calloc((size_t) T + 1, sizeof(int));
  C->fhit = (int *) calloc((size_t) T + 1, sizeof(int));
  C->tracei = (int *) calloc((size_t) T + 1, sizeof(int));
  C->score = (int *) calloc((size_t) T + 1, sizeof(int));
  C->active = (int *) calloc((size_t) T + 1, sizeof(int));
  C->firstactive = (int *) malloc((size_t) querylength * sizeof(int));
  C->splicingp = splicingp;
  C->maxintronlen = (unsigned int) maxintronlen;
  proc = (int *) malloc((size_t) querylength * sizeof(int));
  np = 0;

  /* align_compute_scores_lookforward (stage2.c:4688-5021) */
  q = qend;
  while (q >= 0 && npos[q] <= 0) C->firstactive[q--] = -1;
  if (q >= 0) {
    for (hit = npos[q] - 1; hit >= 0; hit--) {
      LNK(C, fpos, q, hit) = LNK(C, fhit, q, hit) = -1;
      LNK(C, consec, q, hit) = INDEXSIZE;
      LNK(C, tracei, q, hit) = -1;
      LNK(C, score, q, hit) = INDEXSIZE;
    }
    revise_active(C, q, 0, npos[q]);
  }
  grand_score = 0;
  grand_q = grand_hit = -1;
  while (q >= 0) {
    best_score = 0;
    best_hit = -1;
    for (hit = npos[q] - 1; hit >= 0 && MAP(C, q, hit) > chrterm; hit--) ;
    high = hit + 1;
    for (; hit >= 0 && MAP(C, q, hit) >= chrinit; hit--) ;
    low = hit + 1;
    if (high - low >= MAX_NACTIVE) C->cnt[S2S_BIG_POSITION]++;   /* skip_repetitive_p false: scored */
    if (high - low > 0) {
      if (high - low == 1) {
        score_one(C, q, low, proc, np);
        if (LNK(C, score, q, low) > 0) {
          best_score = LNK(C, score, q, low);
          best_hit = low;
        }
      } else {
        score_mult(C, q, low, high, proc, np);
        for (hit = high - 1; hit >= low; hit--)
          if (LNK(C, score, q, hit) > best_score) {
            best_score = LNK(C, score, q, hit);
            best_hit = hit;
          }
      }
      if (best_hit < 0) {   /* middlep false: a new start (:4895-4920), every hit of the position */
        for (hit = 0; hit < npos[q]; hit++) {
          LNK(C, fpos, q, hit) = LNK(C, fhit, q, hit) = -1;
          LNK(C, consec, q, hit) = INDEXSIZE;
          LNK(C, tracei, q, hit) = -1;
          LNK(C, score, q, hit) = INDEXSIZE;
        }
        C->cnt[S2S_RESTART]++;
      }
      /* grand lookforward (stage2.c:4923-4950) */
      if (splicingp && best_hit >= 0 && LNK(C, fhit, q, best_hit) < 0 && grand_q <= querylength - INDEXSIZE &&
          q + INDEXSIZE <= grand_q) {
        if ((best_score = LNK(C, score, grand_q, grand_hit) - (grand_q - q)) > 0) {
          prevposition = MAP(C, grand_q, grand_hit);
          for (hit = high - 1; hit >= low; hit--) {
            position = MAP(C, q, hit);
            if (position + C->maxintronlen < prevposition) {
              /* too long */
            } else if (position + INDEXSIZE <= prevposition) {
              LNK(C, consec, q, hit) = INDEXSIZE;
              LNK(C, fpos, q, hit) = grand_q;
              LNK(C, fhit, q, hit) = grand_hit;
              LNK(C, tracei, q, hit) = ++C->tracectr;
              LNK(C, score, q, hit) = best_score;
            }
          }
        }
      }
      if (best_hit >= 0 && best_score >= grand_score && LNK(C, consec, q, best_hit) > EXON_DEFN) {
        grand_score = best_score;
        grand_q = q;
        grand_hit = best_hit;
      }
    }
    revise_active(C, q, low, high);
    if (npos[q] > 0) proc[np++] = q;
    q--;
  }

  /* get_cells_fwd (stage2.c:3437) */
  cellv = (OCell *) malloc(((size_t) T + 1) * sizeof(OCell));
  cells = (OCell **) malloc(((size_t) T + 1) * sizeof(OCell *));
  sorted = (OCell **) malloc(((size_t) T + 1) * sizeof(OCell *));
  ncells = 0;
  for (q = 0; q <= qend; q++)
    for (hit = 0; hit < npos[q]; hit++)
      if (LNK(C, score, q, hit) > 0) {
        OCell *c = &cellv[ncells];
        c->root = LNK(C, root, q, hit);
        c->endpos = (int) MAP(C, q, hit);
        c->querypos = q;
        c->hit = hit;
        c->score = LNK(C, score, q, hit);
        cells[ncells] = c;
        ncells++;
      }
  for (i = 0; i < ncells / 2; i++) {   /* Cellpool_push prepends: newest cell first */
    OCell *t = cells[i];
    cells[i] = cells[ncells - 1 - i];
    cells[ncells - 1 - i] = t;
  }
  stable_sort((void **) cells, ncells, cell_root_cmp);
  {
    int last_root = -1, best_for_root = -1;
    for (k = 0, i = 0; i < ncells; i++) {
      if (cells[i]->root != last_root) {
        sorted[k++] = cells[i];
        last_root = cells[i]->root;
        best_for_root = cells[i]->score;
      } else if (cells[i]->score == best_for_root) {
        sorted[k++] = cells[i];
      }
    }
  }
  ncells = k;
  stable_sort((void **) sorted, ncells, cell_score_cmp);

  /* the path loop of align_compute_lookforward (stage2.c:5155) with max_nalignments 1 */
  npaths = 0;
  if (ncells > 0) {
    bestscore = sorted[0]->score;
    for (i = 0; i < ncells && (i < MAX_NALIGNMENTS || sorted[i]->score == bestscore) &&
                sorted[i]->score > bestscore - FINAL_SCORE_TOLERANCE; i++)
      npaths++;
  }
  scalars[1] = npaths;
  if (npaths > 1) C->cnt[S2S_TIED_CELLS] += npaths - 1;
  pathq = (int *) malloc(((size_t) querylength + 1) * sizeof(int));
  pathh = (int *) malloc(((size_t) querylength + 1) * sizeof(int));

  {
    OPath *pv = (OPath *) malloc((size_t) (npaths + 1) * sizeof(OPath)), **parr;
    int *elim, nl = 0, any = 0;
    /* all_paths is pushed, walked from its head and each list pushed onto all_results: cell order again; the
       NULL lists are left out */
    for (i = 0; i < npaths; i++) {
      int off0 = sink.n, n = emit_path(C, &sink, sorted[i]->querypos, sorted[i]->hit, queryseq, queryuc, query_offset,
                                        chroffset, chrhigh, plusp, pathq, pathh);
      if (n <= 0 || sink.overflow) continue;
      pv[nl].offset = off0;
      pv[nl].npairs = n;
      pv[nl].end = (unsigned int) sink.p[off0].genomepos;
      pv[nl].start = (unsigned int) sink.p[off0 + n - 1].genomepos;
      nl++;
    }
    /* Stage2pairs_filter_unique_starts (stage2.c:6114) */
    parr = (OPath **) malloc((size_t) (nl + 1) * sizeof(OPath *));
    elim = (int *) calloc((size_t) nl + 1, sizeof(int));
    for (i = 0; i < nl; i++) parr[i] = &pv[i];
    stable_sort((void **) parr, nl, path_cmp);
    for (i = 0; i < nl; i++)
      for (k = i + 1; k < nl; k++)
        if (overlap_p(parr[i], parr[k])) {
          if (!elim[k]) C->cnt[S2S_ELIMINATED]++;
          elim[k] = 1;
          any = 1;
        }
    if (nl > 0 && !any) {   /* "all are identical, so take the first one only" */
      if (nl > 1) C->cnt[S2S_FIRST_KEPT]++;
      if (path_cap > 0) { paths[0] = parr[0]->offset; paths[1] = parr[0]->npairs; }
      nkept = 1;
    } else {
      for (i = 0; i < nl; i++) {
        if (elim[i]) continue;
        if (nkept < path_cap) {
          paths[2 * nkept] = parr[i]->offset;
          paths[2 * nkept + 1] = parr[i]->npairs;
        }
        nkept++;
      }
    }
    free(elim); free(parr); free(pv);
  }
  scalars[0] = nkept;

  free(pathq); free(pathh);
  free(cellv); free(cells); free(sorted); free(proc);
  free(C->consec); free(C->root); free(C->fpos); free(C->fhit); free(C->tracei); free(C->score);
  free(C->active); free(C->firstactive); free((void *) C->off);
  free(npos); free(positions);
  if (sink.overflow || nkept > path_cap) return -1;
  return nkept;
}

int
orc_stage2_starts (const char *queryseq, const char *queryuc, int querylength, int query_offset,
                   unsigned int chrstart, unsigned int chrend, unsigned int chroffset, unsigned int chrhigh, int plusp,
                   int splicingp, int maxintronlen, int *scalars, int *paths, int path_cap, OrcPair *pairs,
                   int pair_cap, long *counters) {
  return stage2s(queryseq, queryuc, querylength, query_offset, chrstart, chrend, chroffset, chrhigh, plusp, splicingp,
                 maxintronlen, scalars, paths, path_cap, pairs, pair_cap, counters);
}

/* n calls on the current genome over `nthreads` threads, in orc_stage2_batch's formats
   (oracle/stage2_chain_oracle.c): call i reads qseq / quc at qoff[i] and writes scalars[8 i ...] = {its return
   value, paths traced, ncovered, status, querystart, queryend, 0, 0}, paths[2 (path_cap i + k) ...] = {first
   record relative to the call's slot, records} of returned list k, and its records from pairs[pair_off[i]] on
   (pair_off[i + 1] - pair_off[i] at most, else scalars[8 i] = -9) in the engine's gmapdp_path_pair layout. */
typedef struct {
  int querypos, genomepos, queryjump, genomejump;
  char cdna, comp, genome, genomealt;
} OrcPathPair;

typedef struct {
  int n;
  const char *qseq, *quc;
  const int *qoff, *qlen, *query_offset, *plusp, *splicingp, *maxintronlen;
  const unsigned int *chrstart, *chrend, *chroffset, *chrhigh;
  int *scalars, *paths, path_cap;
  OrcPathPair *pairs;
  const long *pair_off;
  int next;
  pthread_mutex_t lock;
} S2SBatch;

static void *
s2sbatch_worker (void *arg) {
  S2SBatch *B = (S2SBatch *) arg;
  int *kp = (int *) malloc(2 * (size_t) B->path_cap * sizeof(int));
  for (;;) {
    int i, k, j, r, cap;
    OrcPair *tmp;
    long o;
    int *pp;
    pthread_mutex_lock(&B->lock);
    i = B->next++;
    pthread_mutex_unlock(&B->lock);
    if (i >= B->n) break;
    cap = 64 * B->qlen[i] > (1 << 16) ? 64 * B->qlen[i] : (1 << 16);
    tmp = (OrcPair *) malloc((size_t) cap * sizeof(OrcPair));
    r = stage2s(B->qseq + B->qoff[i], B->quc + B->qoff[i], B->qlen[i], B->query_offset[i], B->chrstart[i],
                B->chrend[i], B->chroffset[i], B->chrhigh[i], B->plusp[i], B->splicingp[i], B->maxintronlen[i],
                B->scalars + 8 * (size_t) i, kp, B->path_cap, tmp, cap, NULL);
    B->scalars[8 * (size_t) i] = r;
    o = B->pair_off[i];
    pp = B->paths + 2 * (size_t) B->path_cap * i;
    for (k = 0; r > 0 && k < r; k++) {
      if (o + kp[2 * k + 1] > B->pair_off[i + 1]) {
        B->scalars[8 * (size_t) i] = -9;
        break;
      }
      pp[2 * k] = (int) (o - B->pair_off[i]);
      pp[2 * k + 1] = kp[2 * k + 1];
      for (j = 0; j < kp[2 * k + 1]; j++, o++) {
        const OrcPair *x = &tmp[kp[2 * k] + j];
        OrcPathPair *y = &B->pairs[o];
        y->querypos = x->querypos;
        y->genomepos = x->genomepos;
        y->queryjump = x->queryjump;
        y->genomejump = x->genomejump;
        y->cdna = x->cdna;
        y->comp = x->comp;
        y->genome = x->genome;
        y->genomealt = x->genomealt;
      }
    }
    free(tmp);
  }
  free(kp);
  return NULL;
}

int
orc_stage2s_batch (int n, const char *qseq, const char *quc, const int *qoff, const int *qlen,
                   const int *query_offset, const unsigned int *chrstart, const unsigned int *chrend,
                   const unsigned int *chroffset, const unsigned int *chrhigh, const int *plusp, const int *splicingp,
                   const int *maxintronlen, int *scalars, int *paths, int path_cap, void *pairs, const long *pair_off,
                   int nthreads) {
  S2SBatch B;
  pthread_t th[64];
  int t;
  if (nthreads < 1) nthreads = 1;
  if (nthreads > 64) nthreads = 64;
  B.n = n; B.qseq = qseq; B.quc = quc; B.qoff = qoff; B.qlen = qlen; B.query_offset = query_offset;
  B.plusp = plusp; B.splicingp = splicingp; B.maxintronlen = maxintronlen; B.chrstart = chrstart; B.chrend = chrend;
  B.chroffset = chroffset; B.chrhigh = chrhigh; B.scalars = scalars; B.paths = paths; B.path_cap = path_cap;
  B.pairs = (OrcPathPair *) pairs; B.pair_off = pair_off; B.next = 0;
  pthread_mutex_init(&B.lock, NULL);
  for (t = 0; t < nthreads; t++) pthread_create(&th[t], NULL, s2sbatch_worker, &B);
  for (t = 0; t < nthreads; t++) pthread_join(th[t], NULL);
  pthread_mutex_destroy(&B.lock);
  return 0;
}
