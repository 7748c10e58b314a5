/* tests/golden/alt_refharness.c -- TEST INFRASTRUCTURE ONLY (golden generation; never shipped).
 *
 * A flat C API over the *reference's own* Dynprog_single_gap (dynprog_single.c:429), Dynprog_end5_gap and
 * Dynprog_end3_gap (dynprog_end.c:1294 / 1924) called with an alternate-allele genome, as gmap --use-snps
 * calls them: a reference Genome_T and an alternate one, each made by Genome_from_sequence (genome.c:307)
 * from its own sequence.  Two distinct block arrays send Genome_get_segment_right / _left and
 * get_genomic_nt down their snps_subst paths.  `use_alt` 0 passes genomealt == genome instead (the runs the
 * generator compares against).  The set-up is oracle/refharness.c's refh_init with the mode as an argument
 * (Dynprog_init builds the score and consistency tables of that mode).  Everything here only *calls*
 * reference functions.  tests/golden/make_alt_golden.py compiles this file against the nosimd objects
 * `make ref` leaves in oracle/_ref/nosimd/ into a temporary directory and writes
 * tests/golden/alt_single_gap_golden.npz and alt_end_gap_golden.npz.
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
#include "mode.h"
#include "dynprog.h"
#include "dynprog_single.h"
#include "dynprog_end.h"

typedef struct {
  int querypos;
  int genomepos;
  int queryjump;
  int genomejump;
  int dynprogindex;
  char cdna, comp, genome, genomealt;
  int gapp;
} RefPair;

static Dynprog_T dynprogM = NULL, dynprogL = NULL, dynprogR = NULL;
static Pairpool_T pairpool = NULL;
static Genome_T genome = NULL, genomealt = NULL;

/* gmap.c:259,275-277 and stage3.h:36 defaults, as oracle/refharness.c */
#define NULLGAP 600
#define EXTRAQUERYGAP 20
#define MAXPEELBACK 60
#define EXTRAMATERIAL_END 10
#define EXTRAMATERIAL_PAIRED 8

/* mode: 0 STANDARD, 1 CMET_STRANDED (mode.h) */
int
alth_init (int mode) {
  Dynprog_init((Mode_T) mode);
  Dynprog_single_setup(0, 0, /*user_dynprog_p*/false, /*homopolymerp*/false);
  Dynprog_end_setup(NULL, NULL, NULL, /*nsplicesites*/0, NULL, NULL, NULL, NULL, 0, 0, /*user_dynprog_p*/false);
  dynprogM = Dynprog_new(NULLGAP, EXTRAQUERYGAP, MAXPEELBACK, EXTRAMATERIAL_END, EXTRAMATERIAL_PAIRED, false);
  dynprogL = Dynprog_new(NULLGAP, EXTRAQUERYGAP, MAXPEELBACK, EXTRAMATERIAL_END, EXTRAMATERIAL_PAIRED, true);
  dynprogR = Dynprog_new(NULLGAP, EXTRAQUERYGAP, MAXPEELBACK, EXTRAMATERIAL_END, EXTRAMATERIAL_PAIRED, true);
  pairpool = Pairpool_new();
  return 0;
}

static Genome_T
wrap (const char *seq, int length) {
  char *copy = (char *) malloc(length + 1);
  Genome_T g;
  memcpy(copy, seq, length);
  copy[length] = '\0';
  g = Genome_from_sequence(Sequence_genomic_new(copy, length, /*copyp*/true));
  free(copy);
  return g;
}

int
alth_set_genomes (const char *refseq, const char *altseq, int length) {
  genome = wrap(refseq, length);
  genomealt = wrap(altseq, length);
  return 0;
}

static int
flatten (List_T pairs, RefPair *out, int max_pairs) {
  int n = 0;
  List_T p;
  for (p = pairs; p != NULL; p = List_next(p)) {
    Pair_T pair = (Pair_T) List_head(p);
    if (n < max_pairs) {
      out[n].querypos = pair->querypos;
      out[n].genomepos = (int) pair->genomepos;
      out[n].queryjump = pair->queryjump;
      out[n].genomejump = pair->genomejump;
      out[n].dynprogindex = pair->dynprogindex;
      out[n].cdna = pair->cdna;
      out[n].comp = pair->comp;
      out[n].genome = pair->genome;
      out[n].genomealt = pair->genomealt;
      out[n].gapp = pair->gapp ? 1 : 0;
    }
    n++;
  }
  return n;
}

/* scalars[0..5] = dynprogindex(after), finalscore, nmatches, nmismatches, nopens, nindels.
   Returns the number of pairs, or -1 when the reference returned NULL. */
int
alth_single_gap (int use_alt, const char *rsequence, const char *rsequenceuc, int rlength, int glength, int roffset,
                 int goffset, unsigned int chroffset, unsigned int chrhigh, int watsonp, int genestrand,
                 int jump_late_p, int extraband_single, int widebandp, double defect_rate, int dynprogindex,
                 int *scalars, RefPair *out, int max_pairs) {
  List_T pairs;
  int finalscore = 0, nmatches = 0, nmismatches = 0, nopens = 0, nindels = 0;

  Pairpool_reset(pairpool);
  pairs = Dynprog_single_gap(&dynprogindex, &finalscore, &nmatches, &nmismatches, &nopens, &nindels, dynprogM,
                             (char *) rsequence, (char *) rsequenceuc, rlength, glength, roffset, goffset,
                             (Univcoord_T) chroffset, (Univcoord_T) chrhigh, watsonp ? true : false, genestrand,
                             jump_late_p ? true : false, genome, use_alt ? genomealt : genome, pairpool,
                             extraband_single, widebandp ? true : false, defect_rate);
  scalars[0] = dynprogindex; scalars[1] = finalscore; scalars[2] = nmatches;
  scalars[3] = nmismatches; scalars[4] = nopens; scalars[5] = nindels;
  return pairs == NULL ? -1 : flatten(pairs, out, max_pairs);
}

/* endalign: 0 QUERYEND_GAP, 1 QUERYEND_INDELS, 2 QUERYEND_NOGAPS, 3 BEST_LOCAL (dynprog.h:23); the query is
   qbuf + qpos (end5: the slice's last character, its rev pointer) */
int
alth_end_gap (int use_alt, int end3p, const char *qbuf, const char *qucbuf, int qpos, int rlength, int glength,
              int roffset, int goffset, unsigned int chroffset, unsigned int chrhigh, int watsonp, int genestrand,
              int jump_late_p, int extraband_end, double defect_rate, int endalign, int require_pos_score_p,
              int dynprogindex, int *scalars, RefPair *out, int max_pairs) {
  List_T pairs;
  int finalscore = 0, nmatches = 0, nmismatches = 0, nopens = 0, nindels = 0;
  const char *rsequence = qbuf + qpos, *rsequenceuc = qucbuf + qpos;
  Genome_T ga = use_alt ? genomealt : genome;

  Pairpool_reset(pairpool);
  if (end3p) {
    pairs = Dynprog_end3_gap(&dynprogindex, &finalscore, &nmatches, &nmismatches, &nopens, &nindels, dynprogR,
                             (char *) rsequence, (char *) rsequenceuc, rlength, glength, roffset, goffset,
                             (Univcoord_T) chroffset, (Univcoord_T) chrhigh, watsonp ? true : false, genestrand,
                             jump_late_p ? true : false, genome, ga, pairpool, extraband_end, defect_rate,
                             (Endalign_T) endalign, require_pos_score_p ? true : false);
  } else {
    pairs = Dynprog_end5_gap(&dynprogindex, &finalscore, &nmatches, &nmismatches, &nopens, &nindels, dynprogL,
                             (char *) rsequence, (char *) rsequenceuc, rlength, glength, roffset, goffset,
                             (Univcoord_T) chroffset, (Univcoord_T) chrhigh, watsonp ? true : false, genestrand,
                             jump_late_p ? true : false, genome, ga, pairpool, extraband_end, defect_rate,
                             (Endalign_T) endalign, require_pos_score_p ? true : false);
  }
  scalars[0] = dynprogindex; scalars[1] = finalscore; scalars[2] = nmatches;
  scalars[3] = nmismatches; scalars[4] = nopens; scalars[5] = nindels;
  return pairs == NULL ? -1 : flatten(pairs, out, max_pairs);
}
