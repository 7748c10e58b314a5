/* tests/golden/stage2_starts_refharness.c -- TEST INFRASTRUCTURE ONLY (golden generation; never shipped).
 *
 * A flat C API over the *reference's own* Stage2_compute_starts (stage2.c:6914), called with the arguments
 * stage 3 passes (stage3.c:15955 / 16166: oligoindices_minor, localp false, skip_repetitive_p false,
 * favor_right_p false, max_nalignments 1; genomealt = genome, genestrand 0) after the set-up of
 * stage2x_refharness.c (Oligoindex_hr_setup(STANDARD), Stage2_setup with cross_species_p false, sufflookback 60,
 * nsufflookback 5, no SNPs).  Everything here only *calls* reference functions.
 * tests/golden/make_stage2_starts.py compiles this file against the reference objects `make ref` leaves in
 * oracle/_ref/nosimd/ into a temporary directory and writes tests/golden/stage2_starts_golden.npz.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bool.h"
#include "mem.h"
#include "list.h"
#include "pair.h"
#include "pairdef.h"
#include "pairpool.h"
#include "sequence.h"
#include "genome.h"
#include "oligoindex_hr.h"
#include "diag.h"
#include "diagpool.h"
#include "cellpool.h"
#include "stage2.h"

typedef struct {
  int querypos;
  int genomepos;
  int queryjump;
  int genomejump;
  int dynprogindex;
  char cdna, comp, genome, genomealt;
  int gapp;
} RefPair;

static Pairpool_T pairpool = NULL;
static Genome_T genome = NULL;
static Sequence_T genome_seq = NULL;
static Oligoindex_array_T oligo_major = NULL, oligo_minor = NULL;
static Diagpool_T diagpool = NULL;
static Cellpool_T cellpool = NULL;
static int stage2_splicingp = -1, stage2_maxintronlen = -1;

int
s2sh_set_genome (const char *seq, int length) {
  char *copy = (char *) malloc(length + 1);
  memcpy(copy, seq, length);
  copy[length] = '\0';
  genome_seq = Sequence_genomic_new(copy, length, /*copyp*/true);
  genome = Genome_from_sequence(genome_seq);
  free(copy);
  return 0;
}

static int
flatten (List_T list, RefPair *pairs, int n, int pair_cap) {
  List_T q;
  for (q = list; q != NULL; q = List_next(q)) {
    Pair_T pr = (Pair_T) List_head(q);
    if (n < pair_cap) {
      RefPair *r = &pairs[n];
      r->querypos = pr->querypos;
      r->genomepos = pr->genomepos;
      r->queryjump = pr->gapp ? pr->queryjump : 0;
      r->genomejump = pr->gapp ? pr->genomejump : 0;
      r->dynprogindex = pr->dynprogindex;
      r->cdna = pr->cdna;
      r->comp = pr->comp;
      r->genome = pr->genome;
      r->genomealt = pr->genomealt;
      r->gapp = pr->gapp ? 1 : 0;
    }
    n++;
  }
  return n;
}

/* Stage2_compute_starts on the query's first `querylength` characters, as stage 3 passes them: a pointer into a
   longer buffer.  paths[2 i] / paths[2 i + 1] = first record / record count of returned list i, each list
   flattened in list order.  Returns the number of lists, -1 when a capacity is too small. */
int
s2sh_compute (const char *queryseq, const char *queryuc, int querylength, int query_offset, unsigned int chrstart,
              unsigned int chrend, unsigned int chroffset, unsigned int chrhigh, int plusp, int splicingp,
              int maxintronlen, int *paths, int path_cap, RefPair *pairs, int pair_cap) {
  List_T p, lists;
  int nres = 0, n = 0, n0;
  if (oligo_major == NULL) {
    Oligoindex_hr_setup(STANDARD);
    oligo_major = Oligoindex_array_new_major(100000, 1000000);  /* gmap.c:113-114, 4739-4740 */
    oligo_minor = Oligoindex_array_new_minor(100000, 1000000);
    diagpool = Diagpool_new();
    cellpool = Cellpool_new();
    pairpool = Pairpool_new();
  }
  if (splicingp != stage2_splicingp || maxintronlen != stage2_maxintronlen) {
    Stage2_setup(splicingp ? true : false, /*cross_species_p*/false, /*suboptimal_score_start*/-1,
                 /*suboptimal_score_end*/3, /*sufflookback*/60, /*nsufflookback*/5, maxintronlen, STANDARD,
                 /*snps_p*/false);
    stage2_splicingp = splicingp;
    stage2_maxintronlen = maxintronlen;
  }
  Pairpool_reset(pairpool);
  lists = Stage2_compute_starts((char *) queryseq, (char *) queryuc, querylength, query_offset, chrstart, chrend,
                                chroffset, chrhigh, plusp ? true : false, /*genestrand*/0, oligo_minor, genome,
                                genome, pairpool, diagpool, cellpool, /*localp*/false,
                                /*skip_repetitive_p*/false, /*favor_right_p*/false, /*max_nalignments*/1);
  for (p = lists; p != NULL; p = List_next(p)) {
    n0 = n;
    n = flatten((List_T) List_head(p), pairs, n, pair_cap);
    if (nres < path_cap) { paths[2 * nres] = n0; paths[2 * nres + 1] = n - n0; }
    nres++;
  }
  List_free(&lists);
  return (nres > path_cap || n > pair_cap) ? -1 : nres;
}
