/* tests/s2xoracle/s2x_oracle.c -- TEST INFRASTRUCTURE ONLY (never shipped, never on the product path).
 *
 * CPU restatement of the two stage-2 entry points stage 3 calls on a query segment (paths under the
 * reference tree's src/):
 *
 *   Stage2_compute_one   stage2.c:6754, as stage3.c:11382 calls it (localp true, skip_repetitive_p false,
 *                        favor_right_p false; middlep true, max_nalignments 1)
 *   Stage2_compute_ends  stage2.c:7087, as stage3.c:15849 / 16068 call it (localp false, skip_repetitive_p
 *                        false, favor_right_p false, max_nalignments 1; middlep false)
 *
 * with use_canonical_middle_p false, genomealt == genome, genestrand 0, mode STANDARD, no SNPs.  The seeding
 * (the minor oligoindex: diag_lookback 60, suffnconsecutive 10) and the genome come from
 * oracle/libgmapdp_oracle.so; the chain is restated here (oracle/stage2_chain_oracle.c's functions are
 * static).  Where the two calls part from Stage2_compute:
 *
 *   no coverage test           they chain whenever totalpositions > 0
 *   Diag_max_bounds            diag.c:894: minactive = chrinit, maxactive = chrterm at every query position,
 *                              querystart 0, queryend querylength - 1
 *   skip_repetitive_p false    stage2.c:3862-3887 never runs: a position with >= MAX_NACTIVE hits is scored
 *   localp false (ENDS)        a hit without a predecessor keeps best_fwd_score (0) where localp stores
 *                              indexsize_nt (:1445-1451, :1993-1999; fwd_tracei advances); in _mult's
 *                              last_item == NULL branch (:1551-1556) the score is 0 and fwd_tracei is not
 *                              advanced (its other two early branches are unreachable: processed ==
 *                              last_item without MOVE_TO_STAGE3)
 *   middlep false (ENDS)       a position none of whose hits scored above 0 restarts: every hit of the
 *                              position gets fwd_pos = fwd_hit = -1, fwd_consecutive 8, fwd_tracei -1, score 8
 *                              (:3955-3980), before the grand lookback and revise_active_lookback
 *   max_nalignments 1          the path loop (:4495) keeps cell 0 and every further cell of the best score
 *   ONE                        List_head(all_paths) = the last cell traced; reversed, converted with gap
 *                              holders; returned as List_reverse(middle): 3' end first
 *   ENDS                       every traced path converted without gap holders, in cell order, then
 *                              Stage2pairs_filter_unique_ends (:6218): stable sort by stage2pairs_end_cmp,
 *                              every list overlapping an earlier one eliminated; nothing eliminated: only
 *                              array[0] is kept
 *   query_offset               added to every pair's querypos (convert_to_nucleotides :5334)
 *
 * glibc's qsort is a stable merge sort for these sizes, so is stable_sort below.  Per call the rules above
 * are counted (S2X_* below).  Pinned against the reference's own two functions by tests/test_stage2x_oracle.py
 * over tests/golden/stage2x_golden.npz.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "gmapdp_oracle.h"

#define KIND_ONE 1
#define KIND_ENDS 2

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
enum { S2X_RESTART, S2X_ZERO_EARLY, S2X_BIG_POSITION, S2X_TIED_CELLS, S2X_ELIMINATED, S2X_FIRST_KEPT, S2X_GAPHOLDER,
       S2X_NCOUNTERS };

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
  int tracectr, splicingp, localp, middlep;
  unsigned int maxintronlen;
  long *cnt;
} Chain;

#define MAP(C, q, h) ((C)->map[(C)->off[q] + (h)])
#define LNK(C, f, q, h) ((C)->f[(C)->off[q] + (h)])

typedef struct {
  int consec, root, pp, ph, score, tracei;
} Best;

/* the tail of score_querypos_lookback_one (:1432-1451) and of _mult's general branch (:1981-1999) */
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
  } else if (C->localp) {
    C->tracei[gi] = ++C->tracectr;
    C->score[gi] = INDEXSIZE;
  } else {
    C->tracei[gi] = ++C->tracectr;
    C->score[gi] = b->score;   /* as the search left it: 0 */
  }
}

static int
score_ranges (Chain *C, Best *b, int q, unsigned int position, int pq, int ph, int *last_tr, int range1) {
  int qd = q - pq, credit = -qd / INDEXSIZE, gendist, diff, fs, frontier;
  unsigned int pp;
  while (ph != -1 && LNK(C, tracei, pq, ph) == *last_tr) ph = LNK(C, active, pq, ph);   /* range 0 */
  if (ph != -1) *last_tr = LNK(C, tracei, pq, ph);
  if (range1)
    while (ph != -1 && MAP(C, pq, ph) + C->maxintronlen + (unsigned int) qd <= position) ph = LNK(C, active, pq, ph);
  frontier = ph;
  while (ph != -1 && (pp = MAP(C, pq, ph)) + EQUAL_DISTANCE_NOT_SPLICING + (unsigned int) qd < position) {
    gendist = (int) (position - pp);
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
  while (ph != -1 && (pp = MAP(C, pq, ph)) + INDEXSIZE <= position) {   /* ranges 3-4 */
    gendist = (int) (position - pp);
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

static int
adjacent (Chain *C, int pq, int *ph_io, int qd, unsigned int position) {
  int ph = *ph_io;
  unsigned int pp = position;
  while (ph != -1 && (pp = MAP(C, pq, ph)) + (unsigned int) qd < position) ph = LNK(C, active, pq, ph);
  *ph_io = ph;
  return pp + (unsigned int) qd == position;
}

/* score_querypos_lookback_one (stage2.c:1073); proc[0..np) oldest first */
static void
score_one (Chain *C, int q, int hit, const int *proc, int np) {
  unsigned int position = MAP(C, q, hit);
  Best b = {INDEXSIZE, (int) position, -1, -1, 0, 0};
  int nlookback = NSUFFLOOKBACK, lookback = SUFFLOOKBACK, k, nseen, donep, last_tr, pq, qd, ph;
  if (np > 0) {
    pq = proc[np - 1];
    qd = q - pq;
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
    qd = q - pq;
    if (nseen > nlookback && qd - INDEXSIZE > lookback) donep = 1;
    if ((ph = C->firstactive[pq]) != -1) score_ranges(C, &b, q, position, pq, ph, &last_tr, C->splicingp);
  }
  finish_link(C, q, hit, &b);
}

/* score_querypos_lookback_mult (stage2.c:1470) over hits [low, high) */
static void
score_mult (Chain *C, int q, int low, int high, const int *proc, int np) {
  int nhits = high - low, hiti, adj, adq, n, maxadj = 0, maxnon = 0, overall = 0, adjf, ph, maxseen, nseen, k,
      last_tr, pq, qd;
  int *frontier;
  unsigned int position;
  Best b;
  if (np == 0) {   /* last_item == NULL (:1536-1557) */
    for (hiti = 0; hiti < nhits; hiti++) {
      int gi = C->off[q] + low + hiti;
      C->consec[gi] = INDEXSIZE;
      C->root[gi] = (int) MAP(C, q, low + hiti);
      C->fpos[gi] = C->fhit[gi] = -1;
      if (C->localp) {
        C->tracei[gi] = ++C->tracectr;
        C->score[gi] = INDEXSIZE;
      } else {
        C->score[gi] = 0;   /* fwd_tracei keeps what it held */
        C->cnt[S2X_ZERO_EARLY]++;
      }
    }
    return;
  }
  adj = proc[np - 1];
  adq = q - adj;
  frontier = (int *) malloc((size_t) np * sizeof(int));
  for (n = 0; n < np; n++) {
    qd = q - proc[np - 1 - n];
    if (n <= 1 || qd - INDEXSIZE <= SUFFLOOKBACK / 2) maxadj = n;
    if (n <= NSUFFLOOKBACK || qd - INDEXSIZE <= SUFFLOOKBACK) maxnon = n;
    frontier[n] = C->firstactive[proc[np - 1 - n]];
  }
  adjf = C->firstactive[adj];
  for (hiti = 0; hiti < nhits; hiti++) {
    position = MAP(C, q, low + hiti);
    ph = adjf;
    if (adjacent(C, adj, &ph, adq, position) && LNK(C, consec, adj, ph) + adq > overall)
      overall = LNK(C, consec, adj, ph) + adq;
    adjf = ph;
  }
  adjf = C->firstactive[adj];
  for (hiti = 0; hiti < nhits; hiti++) {
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

/* revise_active_lookback (stage2.c:2956) */
static void
revise_active (Chain *C, int q, int low, int high) {
  int best, threshold, hit, *ptr;
  if (low >= high) {
    C->firstactive[q] = -1;
    return;
  }
  best = LNK(C, score, q, low);
  for (hit = low + 1; hit < high; hit++)
    if (LNK(C, score, q, hit) > best) best = LNK(C, score, q, hit);
  threshold = best - SCORE_FOR_RESTRICT;
  if (threshold < 0) threshold = 0;
  C->firstactive[q] = -1;
  ptr = &C->firstactive[q];
  hit = low;
  while (hit < high) {
    while (hit < high && LNK(C, score, q, hit) <= threshold) hit++;
    *ptr = hit;
    if (hit < high) {
      ptr = &LNK(C, active, q, hit);
      hit++;
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

static void
gapholder (Sink *s, int queryjump, int genomejump) {  /* Pairpool_push_gapholder (pairpool.c:375) */
  OrcPair *r;
  if (s->n >= s->cap) { s->overflow = 1; return; }
  r = &s->p[s->n++];
  memset(r, 0, sizeof(*r));
  r->querypos = r->genomepos = -1;
  r->queryjump = queryjump;
  r->genomejump = genomejump;
  r->cdna = r->comp = r->genome = r->genomealt = ' ';
  r->gapp = 1;
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

/* traceback_one (stage2.c:4140) + List_reverse + convert_to_nucleotides (stage2.c:5334) of the path ending in
   cell (q, hit).  The records are appended in the order convert_to_nucleotides pushes them (3' end first);
   ascending: flipped to the list it returns (5' end first).  Returns the number of records appended. */
static int
emit_path (Chain *C, Sink *s, int q, int hit, const char *queryseq, const char *queryuc, int query_offset,
           unsigned int chroffset, unsigned int chrhigh, int plusp, int gapholders, int ascending, int *pathq,
           int *pathh) {
  int n = 0, pq, i, start = s->n, lastq, lastg, qj, gj, fill, querypos, genomepos;
  char c;
  while (q >= 0 && LNK(C, consec, q, hit) < MIN_TERMINAL_NCONSECUTIVE) {   /* prune the 3' end */
    pq = q;
    q = LNK(C, fpos, pq, hit);
    hit = LNK(C, fhit, pq, hit);
  }
  while (q >= 0) {
    if ((int) MAP(C, q, hit) >= 0) { pathq[n] = q; pathh[n] = hit; n++; }
    pq = q;
    q = LNK(C, fpos, pq, hit);
    hit = LNK(C, fhit, pq, hit);
  }
  if (n == 0) return 0;
  querypos = pathq[0];
  genomepos = (int) MAP(C, pathq[0], pathh[0]);
  for (lastq = querypos + INDEXSIZE - 1, lastg = genomepos + INDEXSIZE - 1; lastq > querypos; lastq--, lastg--) {
    c = genomic_nt((unsigned int) lastg, chroffset, chrhigh, plusp);
    push(s, lastq + query_offset, lastg, queryseq[lastq], '|', c, c);
  }
  push(s, querypos + query_offset, genomepos, queryseq[querypos], '|', queryuc[querypos], queryuc[querypos]);
  lastq = querypos;
  lastg = genomepos;
  for (i = 1; i < n; i++) {
    querypos = pathq[i];
    genomepos = (int) MAP(C, pathq[i], pathh[i]);
    qj = lastq - 1 - querypos;
    gj = lastg - 1 - genomepos;
    if (qj != 0 || gj != 0) {
      if (querypos + INDEXSIZE - 1 >= lastq || genomepos + INDEXSIZE - 1 >= lastg)
        fill = (lastq - querypos < lastg - genomepos) ? lastq - querypos - 1 : lastg - genomepos - 1;
      else
        fill = INDEXSIZE - 1;
      qj -= fill;
      gj -= fill;
      if (gapholders && (gj > 0 || qj > 0)) {
        gapholder(s, qj, gj);
        C->cnt[S2X_GAPHOLDER]++;
      }
      for (lastq = querypos + fill, lastg = genomepos + fill; lastq > querypos; lastq--, lastg--) {
        c = genomic_nt((unsigned int) lastg, chroffset, chrhigh, plusp);
        push(s, lastq + query_offset, lastg, queryseq[lastq], '|', c, c);
      }
    }
    push(s, querypos + query_offset, genomepos, queryseq[querypos], '|', queryuc[querypos], queryuc[querypos]);
    lastq = querypos;
    lastg = genomepos;
  }
  if (ascending)
    for (i = start, n = s->n - 1; i < n; i++, n--) {
      OrcPair t = s->p[i];
      s->p[i] = s->p[n];
      s->p[n] = t;
    }
  return s->n - start;
}

typedef struct {
  int offset, npairs;
  unsigned int start, end;    /* genomepos of the first and last pair */
} OPath;

static int
path_cmp (const void *x, const void *y) {   /* stage2pairs_end_cmp (stage2.c:5804) */
  const OPath *a = *(OPath * const *) x, *b = *(OPath * const *) y;
  if (a->start != b->start) return a->start < b->start ? -1 : 1;
  if (a->end != b->end) return a->end < b->end ? -1 : 1;
  return 0;
}

/* stage2pairs_overlap_p (stage2.c:5925) */
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
   list's order; counters[S2X_NCOUNTERS] (may be NULL) are added to.  Returns the number of lists, -1 when a
   capacity is too small, the seeding's error (< -1) otherwise. */
static int
stage2x (int kind, const char *queryseq, const char *queryuc, int querylength, int query_offset,
         unsigned int chrstart, unsigned int chrend, unsigned int chroffset, unsigned int chrhigh, int plusp,
         int splicingp, int maxintronlen, int *scalars, int *paths, int path_cap, OrcPair *pairs, int pair_cap,
         long *counters) {
  int *npos, sc[4], *dg, nd, T, i, q, hit, ncovered, count, *cover, qend, low, high, best_hit, best_score,
      grand_score, grand_q, grand_hit, *proc, np, ncells, k, bestscore, npaths, nkept = 0, *pathq, *pathh, rc;
  unsigned int *positions, chrinit, chrterm, position, prevposition;
  long nocount[S2X_NCOUNTERS];
  Chain Cst, *C = &Cst;
  OCell *cellv, **cells, **sorted;
  Sink sink = {pairs, 0, pair_cap, 0};
  int pos_cap = 1 << 22, diag_cap = 1 << 16;

  for (i = 0; i < 6; i++) scalars[i] = 0;
  if (kind != KIND_ONE && kind != KIND_ENDS) return -5;
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
  C->localp = kind == KIND_ONE;
  C->middlep = kind == KIND_ONE;
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

  /* align_compute_scores_lookback (stage2.c:3746-4080) */
  q = 0;
  while (q <= qend && npos[q] <= 0) C->firstactive[q++] = -1;
  if (q <= qend) {
    for (hit = 0; hit < npos[q]; hit++) {
      LNK(C, fpos, q, hit) = LNK(C, fhit, q, hit) = -1;
      LNK(C, consec, q, hit) = INDEXSIZE;
      LNK(C, tracei, q, hit) = -1;
      LNK(C, score, q, hit) = INDEXSIZE;
    }
    revise_active(C, q, 0, npos[q]);
  }
  grand_score = 0;
  grand_q = grand_hit = -1;
  while (q <= qend) {
    best_score = 0;
    best_hit = -1;
    for (hit = 0; hit < npos[q] && MAP(C, q, hit) < chrinit; hit++) ;
    low = hit;
    for (; hit < npos[q] && MAP(C, q, hit) <= chrterm; hit++) ;
    high = hit;
    if (high - low >= MAX_NACTIVE) C->cnt[S2X_BIG_POSITION]++;   /* skip_repetitive_p false: scored */
    if (high - low > 0) {
      if (high - low == 1) {
        score_one(C, q, low, proc, np);
        if (LNK(C, score, q, low) > 0) {
          best_score = LNK(C, score, q, low);
          best_hit = low;
        }
      } else {
        score_mult(C, q, low, high, proc, np);
        for (hit = low; hit < high; hit++)
          if (LNK(C, score, q, hit) > best_score) {
            best_score = LNK(C, score, q, hit);
            best_hit = hit;
          }
      }
      if (!C->middlep && best_hit < 0) {   /* a new start (:3955-3980): every hit of the position */
        for (hit = 0; hit < npos[q]; hit++) {
          LNK(C, fpos, q, hit) = LNK(C, fhit, q, hit) = -1;
          LNK(C, consec, q, hit) = INDEXSIZE;
          LNK(C, tracei, q, hit) = -1;
          LNK(C, score, q, hit) = INDEXSIZE;
        }
        C->cnt[S2X_RESTART]++;
      }
      /* grand lookback (stage2.c:3983-4009) */
      if (splicingp && best_hit >= 0 && LNK(C, fhit, q, best_hit) < 0 && grand_q >= 0 && q >= grand_q + INDEXSIZE) {
        if ((best_score = LNK(C, score, grand_q, grand_hit) - (q - grand_q)) > 0) {
          prevposition = MAP(C, grand_q, grand_hit);
          for (hit = low; hit < high; hit++) {
            position = MAP(C, q, hit);
            if (position > prevposition + C->maxintronlen) {
              /* too long */
            } else if (position >= prevposition + INDEXSIZE) {
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
    q++;
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

  /* the path loop of align_compute_lookback (stage2.c:4495) with max_nalignments 1 */
  npaths = 0;
  if (ncells > 0) {
    bestscore = sorted[0]->score;
    for (i = 0; i < ncells && (i < MAX_NALIGNMENTS || sorted[i]->score == bestscore) &&
                sorted[i]->score > bestscore - FINAL_SCORE_TOLERANCE; i++)
      npaths++;
  }
  scalars[1] = npaths;
  if (npaths > 1) C->cnt[S2X_TIED_CELLS] += npaths - 1;
  pathq = (int *) malloc(((size_t) querylength + 1) * sizeof(int));
  pathh = (int *) malloc(((size_t) querylength + 1) * sizeof(int));

  if (kind == KIND_ONE) {
    /* List_head(all_paths): the last cell traced; gap holders; List_reverse(middle): 3' end first */
    if (npaths > 0) {
      int n = emit_path(C, &sink, sorted[npaths - 1]->querypos, sorted[npaths - 1]->hit, queryseq, queryuc,
                        query_offset, chroffset, chrhigh, plusp, /*gapholders*/1, /*ascending*/0, pathq, pathh);
      if (n > 0) {
        if (path_cap > 0) { paths[0] = 0; paths[1] = n; }
        nkept = 1;
      }
    }
  } else {
    OPath *pv = (OPath *) malloc((size_t) (npaths + 1) * sizeof(OPath)), **parr;
    int *elim, nl = 0, any = 0;
    for (i = 0; i < npaths; i++) {   /* all_results: the converted lists in cell order, NULL ones left out */
      int off0 = sink.n, n = emit_path(C, &sink, sorted[i]->querypos, sorted[i]->hit, queryseq, queryuc, query_offset,
                                        chroffset, chrhigh, plusp, /*gapholders*/0, /*ascending*/1, pathq, pathh);
      if (n <= 0 || sink.overflow) continue;
      pv[nl].offset = off0;
      pv[nl].npairs = n;
      pv[nl].start = (unsigned int) sink.p[off0].genomepos;
      pv[nl].end = (unsigned int) sink.p[off0 + n - 1].genomepos;
      nl++;
    }
    /* Stage2pairs_filter_unique_ends (stage2.c:6218) */
    parr = (OPath **) malloc((size_t) (nl + 1) * sizeof(OPath *));
    elim = (int *) calloc((size_t) nl + 1, sizeof(int));
    for (i = 0; i < nl; i++) parr[i] = &pv[i];
    stable_sort((void **) parr, nl, path_cmp);
    for (i = 0; i < nl; i++)
      for (k = i + 1; k < nl; k++)
        if (overlap_p(parr[i], parr[k])) {
          if (!elim[k]) C->cnt[S2X_ELIMINATED]++;
          elim[k] = 1;
          any = 1;
        }
    if (nl > 0 && !any) {   /* "all are identical, so take the first one only" */
      if (nl > 1) C->cnt[S2X_FIRST_KEPT]++;
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
orc_stage2_one (const char *queryseq, const char *queryuc, int querylength, int query_offset, unsigned int chrstart,
                unsigned int chrend, unsigned int chroffset, unsigned int chrhigh, int plusp, int splicingp,
                int maxintronlen, int *scalars, int *paths, int path_cap, OrcPair *pairs, int pair_cap,
                long *counters) {
  return stage2x(KIND_ONE, queryseq, queryuc, querylength, query_offset, chrstart, chrend, chroffset, chrhigh, plusp,
                 splicingp, maxintronlen, scalars, paths, path_cap, pairs, pair_cap, counters);
}

int
orc_stage2_ends (const char *queryseq, const char *queryuc, int querylength, int query_offset, unsigned int chrstart,
                 unsigned int chrend, unsigned int chroffset, unsigned int chrhigh, int plusp, int splicingp,
                 int maxintronlen, int *scalars, int *paths, int path_cap, OrcPair *pairs, int pair_cap,
                 long *counters) {
  return stage2x(KIND_ENDS, queryseq, queryuc, querylength, query_offset, chrstart, chrend, chroffset, chrhigh, plusp,
                 splicingp, maxintronlen, scalars, paths, path_cap, pairs, pair_cap, counters);
}

/* n calls of one kind on the current genome over `nthreads` threads, in orc_stage2_batch's formats
   (oracle/stage2_chain_oracle.c): call i reads qseq / quc at qoff[i] and writes scalars[8 i ...] = {its return
   value, paths traced, ncovered, status, querystart, queryend, 0, 0}, paths[2 (path_cap i + k) ...] = {first
   record relative to the call's slot, records} of returned list k, and its records from pairs[pair_off[i]] on
   (pair_off[i + 1] - pair_off[i] at most, else scalars[8 i] = -9) in the engine's gmapdp_path_pair layout. */
typedef struct {
  int querypos, genomepos, queryjump, genomejump;
  char cdna, comp, genome, genomealt;
} OrcPathPair;

typedef struct {
  int n, kind;
  const char *qseq, *quc;
  const int *qoff, *qlen, *query_offset, *plusp, *splicingp, *maxintronlen;
  const unsigned int *chrstart, *chrend, *chroffset, *chrhigh;
  int *scalars, *paths, path_cap;
  OrcPathPair *pairs;
  const long *pair_off;
  int next;
  pthread_mutex_t lock;
} S2XBatch;

static void *
s2xbatch_worker (void *arg) {
  S2XBatch *B = (S2XBatch *) arg;
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
    r = stage2x(B->kind, B->qseq + B->qoff[i], B->quc + B->qoff[i], B->qlen[i], B->query_offset[i], B->chrstart[i],
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
orc_stage2x_batch (int kind, int n, const char *qseq, const char *quc, const int *qoff, const int *qlen,
                   const int *query_offset, const unsigned int *chrstart, const unsigned int *chrend,
                   const unsigned int *chroffset, const unsigned int *chrhigh, const int *plusp, const int *splicingp,
                   const int *maxintronlen, int *scalars, int *paths, int path_cap, void *pairs, const long *pair_off,
                   int nthreads) {
  S2XBatch B;
  pthread_t th[64];
  int t;
  if (nthreads < 1) nthreads = 1;
  if (nthreads > 64) nthreads = 64;
  B.n = n; B.kind = kind; B.qseq = qseq; B.quc = quc; B.qoff = qoff; B.qlen = qlen; B.query_offset = query_offset;
  B.plusp = plusp; B.splicingp = splicingp; B.maxintronlen = maxintronlen; B.chrstart = chrstart; B.chrend = chrend;
  B.chroffset = chroffset; B.chrhigh = chrhigh; B.scalars = scalars; B.paths = paths; B.path_cap = path_cap;
  B.pairs = (OrcPathPair *) pairs; B.pair_off = pair_off; B.next = 0;
  pthread_mutex_init(&B.lock, NULL);
  for (t = 0; t < nthreads; t++) pthread_create(&th[t], NULL, s2xbatch_worker, &B);
  for (t = 0; t < nthreads; t++) pthread_join(th[t], NULL);
  pthread_mutex_destroy(&B.lock);
  return 0;
}
