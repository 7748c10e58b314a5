/* include/gmapdp.h -- C ABI of the MI355X GMAP Dynprog engine (libgmapdp.so).
 *
 * This is the drop-in boundary for GMAP's Dynprog_* hot path.  It is a
 * batched, plain-pointer restatement of the reference entry points; the
 * reference-signature wrappers (Dynprog_single_gap(...) etc., which take
 * GMAP's Dynprog_T / Genome_T / Pairpool_T and return List_T of Pair_T) are
 * declared in include/gmapdp_dynprog.h and documented in INTEGRATION.md.
 *
 * Entry point -> reference interface it replaces (paths under the reference
 * tree's src/):
 *   gmapdp_create            Dynprog_init (dynprog.c:1008) + Dynprog_single_setup
 *                            (dynprog_single.c:101) + Dynprog_end_setup (dynprog_end.c)
 *   gmapdp_destroy           Dynprog_term (dynprog.c:1203)
 *   gmapdp_pack_genome       Compress_create_blocks_comp (compress-write.c:754): the
 *                            .genomecomp block format that GMAP mmaps (genome.c:208)
 *   gmapdp_set_genome        Genome_new / Genome_from_sequence (genome.c:208/307):
 *                            the packed genome is made resident in HBM
 *   gmapdp_single_gap_batch  Dynprog_single_gap (dynprog_single.c:429), one call per
 *                            problem, many problems per launch
 *   gmapdp_end_gap_batch     Dynprog_end5_gap / Dynprog_end3_gap (dynprog_end.c:1294/1924)
 *   gmapdp_genome_gap_batch  Dynprog_genome_gap (dynprog_genome.c:3288) + Dynprog_genome_setup
 *                            (:192, no splicing IIT); gmapdp_genome_splice_sites lists the
 *                            Maxent_hr_*_prob calls (maxent_hr.c:27357-27600) whose values it takes
 *   gmapdp_plan_*            the same calls, planned once and replayed on device-resident
 *                            inputs (mixed single + end batches)
 *   gmapdp_compute_bands     Dynprog_compute_bands (dynprog.c:1247)
 *   gmapdp_cdna_gap_batch    Dynprog_cdna_gap (dynprog_cdna.c:787)
 *   gmapdp_end_splicejunction_batch  Dynprog_end5/3_splicejunction (dynprog_end.c:1653/2249), the
 *                            known-splice-site end alignments of Dynprog_end5/3_known (:2748/3009)
 *   gmapdp_oligo_mappings_batch  stage-2 seeding: Oligoindex_hr_tally + Oligoindex_get_mappings
 *                            (oligoindex_hr.c:33849/34127) as Stage2_compute calls them (stage2.c:6480-6495)
 *   gmapdp_stage2_scan_batch Stage2_scan (stage2.c:5610): the seeding with the major index and
 *                            Diag_update_coverage (diag.c:216), one 16-byte result per gregion
 *   gmapdp_stage2_batch      Stage2_compute (stage2.c:6325) as GMAP calls it (gmap.c:1208): the
 *                            seeding above, then Diag_compute_bounds (diag.c:597),
 *                            align_compute_lookback (stage2.c:4402), convert_to_nucleotides (:5334)
 *                            and Stage2_filter_unique (:6013)
 *   gmapdp_stage2x_batch     Stage2_compute_one (stage2.c:6754), Stage2_compute_ends (:7087) and
 *                            Stage2_compute_starts (:6914) as stage 3 calls them on a query segment
 *                            (stage3.c:11382 / 15849 / 15955): the seeding with the minor index,
 *                            Diag_max_bounds (diag.c:894), align_compute_lookback without skip_repetitive_p
 *                            (ENDS: localp and middlep false; STARTS: the same with
 *                            align_compute_lookforward, :5062), convert_to_nucleotides with query_offset,
 *                            ENDS / STARTS: Stage2pairs_filter_unique_ends / _starts (:6218 / :6114)
 *
 * Semantics: every result is bit-identical to the reference's nosimd build
 * (Dynprog_standard + Dynprog_traceback_std), or with GMAPDP_SIMD to its SIMD builds
 * (dynprog_simd.c); stage-2 seeding has one semantics (both builds agree); see DESIGN.md "Parity".
 *
 * Errors: functions return 0 on success and a negative GMAPDP_E* code on
 * failure (no errno).  A per-problem NULL result (the reference returning a
 * NULL List_T) is reported as npairs == 0 with the reference's score
 * convention in traceback_score (NEG_INFINITY_32 = -32768 for the size
 * guard).
 *
 * Threading: a gmapdp_ctx and its plans are NOT thread-safe.  A context (its
 * scratch buffers, fork/join events and side streams) and every plan created on
 * it must be used by one host thread at a time, and a plan must not run on two
 * streams at once (its pool counter and the context scratch are shared).  Use
 * one context per thread, or serialise.  The GMAP shim gives each of its
 * dispatcher threads its own context (gmapdp_create_ex: one stream each, DP
 * dispatchers at high priority, stage-2 dispatchers at low priority) and
 * uploads the genome to HBM once: the other contexts share that copy
 * (gmapdp_share_genome), so GRCh38 costs 1.16 GB of HBM and a 17-Gnt genome
 * 6.4 GB whatever the number of dispatchers.
 */
#ifndef GMAPDP_H
#define GMAPDP_H

#include <stddef.h>
#include <stdint.h>

/* A universal genome coordinate (GMAP's Univcoord_T, univcoord.h:9-11): 64 bits so that one ABI
 * serves gmap (32-bit Univcoord_T) and gmapl (LARGE_GENOMES, genomes past 2^32 nt).  Chromosome
 * positions (Chrpos_T) stay 32-bit, as in both GMAP builds. */
typedef uint64_t gmapdp_coord_t;

#ifdef __cplusplus
extern "C" {
#endif

#define GMAPDP_OK 0
#define GMAPDP_EINVAL (-1)
#define GMAPDP_ENODEV (-2)
#define GMAPDP_ENOMEM (-3)
#define GMAPDP_ELAUNCH (-4)
#define GMAPDP_ENOGENOME (-5)

/* Reference limits (Dynprog_new with gmap.c defaults, dynprog.c:602-627). */
#define GMAPDP_MAX_RLENGTH 660
#define GMAPDP_MAX_GLENGTH 2000
#define GMAPDP_NEG_INFINITY_32 (-32768)

typedef struct gmapdp_ctx gmapdp_ctx;

/* One Pair_T (pairdef.h:8-42) as the engine emits it, in the order of the
 * List_T the reference returns.  A gap holder (Pairpool_push_gapholder,
 * pairpool.c:375) has querypos == genomepos == -1 and jump == genomejump;
 * ordinary pairs have jump == 0.  dynprogindex is per problem (all pairs of
 * one call carry the caller's *dynprogindex, gap holders carry 0). */
typedef struct {
  int32_t querypos;
  int32_t genomepos;
  int32_t jump;
  char cdna;
  char comp;
  char genome;
  char genomealt;
} gmapdp_pair;

/* Problem flags */
#define GMAPDP_WATSON     0x1  /* watsonp */
#define GMAPDP_JUMP_LATE  0x2  /* jump_late_p */
#define GMAPDP_WIDEBAND   0x4  /* widebandp */
/* Reproduce the reference's SIMD builds (gmap.sse42/.avx2/.avx512, dynprog_simd.c) instead of
 * the nosimd build (Dynprog_standard): Dynprog_simd_8/16 for single gaps, the
 * Dynprog_simd_8/16_upper/_lower triangles with their endpoint scans, bridge and tracebacks for
 * end and genome gaps.  Valid in every problem family (genome gaps: in `flags` as well).  The
 * SIMD fills read arena cells the call never wrote; the engine defines those as zero (a fresh
 * arena).  End gaps with rlength > glength + 1 (chopped lengths, QUERYEND_NOGAPS excepted) are
 * GMAPDP_EINVAL: the reference's lower-triangle scan reads uninitialised scores there. */
#define GMAPDP_SIMD       0x40

/* One Dynprog_single_gap call (dynprog_single.c:429 argument list).  The
 * query slice is qseq[qoff .. qoff+rlength) (rsequence, case as given) and
 * qseq_uc[...] (rsequenceuc) in the batch's query arena. */
typedef struct {
  int32_t qoff;
  int32_t rlength;
  int32_t glength;
  int32_t roffset;
  int32_t goffset;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t flags;          /* GMAPDP_WATSON | GMAPDP_JUMP_LATE | GMAPDP_WIDEBAND */
  int32_t genestrand;     /* 0, +1, +2 */
  int32_t extraband;      /* extraband_single */
  double defect_rate;
  int32_t dynprogindex;   /* *dynprogindex on entry */
  int32_t pad_;
} gmapdp_single_problem;

/* Endalign_T (dynprog.h:25) */
#define GMAPDP_QUERYEND_GAP     0
#define GMAPDP_QUERYEND_INDELS  1
#define GMAPDP_QUERYEND_NOGAPS  2
#define GMAPDP_BEST_LOCAL       3

/* One Dynprog_end5_gap (end3p = 0, dynprog_end.c:1294) or Dynprog_end3_gap
 * (end3p = 1, dynprog_end.c:1924) call.  The query slice is
 * qseq[qoff .. qoff+rlength): for end3 the reference's rsequence points at its
 * first character, for end5 rev_rsequence points at its LAST character (the
 * DP walks away from the anchor).  roffset/goffset are the reference's
 * (rev_)roffset/(rev_)goffset.  The engine applies the reference's chopping
 * to 660 x 2000 (except QUERYEND_NOGAPS). */
typedef struct {
  int32_t qoff;
  int32_t rlength;
  int32_t glength;
  int32_t roffset;
  int32_t goffset;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t flags;          /* GMAPDP_WATSON | GMAPDP_JUMP_LATE */
  int32_t genestrand;
  int32_t extraband;      /* extraband_end */
  int32_t end3p;
  int32_t endalign;       /* GMAPDP_QUERYEND_* / GMAPDP_BEST_LOCAL */
  int32_t require_pos_score_p;
  int32_t dynprogindex;
  double defect_rate;
} gmapdp_end_problem;

/* Per-problem outputs (the reference's out-parameters). */
typedef struct {
  int32_t npairs;          /* 0 <=> NULL List_T */
  int32_t pair_offset;     /* first pair in the batch's pair arena */
  int32_t traceback_score; /* *finalscore / *traceback_score */
  int32_t nmatches;
  int32_t nmismatches;
  int32_t nopens;
  int32_t nindels;
  int32_t dynprogindex;    /* *dynprogindex on exit */
} gmapdp_result;

/* Dynprog_genome_gap flags (in addition to GMAPDP_WATSON / GMAPDP_JUMP_LATE) */
#define GMAPDP_HALFP   0x8
#define GMAPDP_FINALP  0x10
/* Known splice sites (gmap -s with a splice-site file: Dynprog_genome_setup with a splicing IIT and
 * donor/acceptor types, novel splicing on; get_known_splicesites, dynprog_genome.c:405).  The problem's
 * flags per position are in the batch's known-site arena at known_offset (one byte each, 0 or 1):
 *   [0, glengthL)                        the bridge's left_known (dynprog_genome.c:2938-2942)
 *   [glengthL, glengthL + glengthR)      its right_known
 *   then rlength + 1 bytes, then rlength + 1 bytes: genome_gap_simple's left_known / right_known
 *   (:3045-3049, queried with glength = rlength)
 * A known position scores KNOWN_SPLICESITE_REWARD in genome_gap_simple and has probability 1.0; the
 * probability arena then holds the MaxEnt values at every position (known or not).  Both builds'
 * semantics (with GMAPDP_SIMD the SIMD bridge reads the same flags). */
#define GMAPDP_KNOWN_SITES 0x80

/* One Dynprog_genome_gap call (dynprog_genome.c:3288 argument list).  The
 * query slice is qseq[qoff .. qoff+rlength) (rsequence / rsequenceuc).
 * chrnum is not needed (it only serves known-splice-site IIT lookups, which
 * the engine does not perform: see splice probabilities below).
 * Domain: glengthL and glengthR must exceed rlength (every stage3.c call
 * passes queryjump + extramaterial_paired); outside it the reference reads
 * uninitialised probabilities (dynprog_genome.c:2575-2660 leave the last
 * entry unset), so the engine rejects such a batch with GMAPDP_EINVAL.
 *
 * Splice probabilities.  The reference's bridge (dynprog_genome.c:2569-2660)
 * and genome_gap_simple (:3171) read MaxEnt splice-site probabilities
 * (Maxent_hr_*_prob, maxent_hr.c, a host symbol the Dynprog objects import).
 * The caller supplies them in a double arena: problem i's left
 * probabilities at [prob_offset, prob_offset + glengthL) and its right ones
 * at [prob_offset + glengthL, prob_offset + glengthL + glengthR);
 * gmapdp_genome_splice_sites lists the (position, model) of every entry. */
typedef struct {
  int32_t qoff;
  int32_t rlength;
  int32_t glengthL;
  int32_t glengthR;
  int32_t roffset;
  int32_t goffsetL;
  int32_t rev_goffsetR;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t flags;          /* GMAPDP_WATSON | GMAPDP_JUMP_LATE | GMAPDP_HALFP | GMAPDP_FINALP */
  int32_t cdna_direction;
  int32_t genestrand;
  int32_t extraband;      /* extraband_paired (+ peeled indels, stage3.c:9538) */
  int32_t maxpeelback;
  int32_t dynprogindex;
  int32_t known_offset;   /* with GMAPDP_KNOWN_SITES: the problem's first byte in the known-site arena */
  double defect_rate;
  int64_t prob_offset;
} gmapdp_genome_problem;

/* Out-parameters of Dynprog_genome_gap.  new_leftgenomepos,
 * new_rightgenomepos and exonhead are GMAPDP_UNSET where the reference does
 * not write them.  The intron gap holder (Pairpool_push_gapholder with
 * queryjump, genomejump, introntype, donor_prob = left_prob, acceptor_prob =
 * right_prob; dynprog_genome.c:3227-3232 / 3859-3865) is pairs[gap_index]
 * (gap_index -1 for a NULL result); its record carries jump = genomejump. */
#define GMAPDP_UNSET ((int32_t)0x80000000)
typedef struct {
  int32_t npairs;          /* 0 <=> NULL List_T */
  int32_t pair_offset;
  int32_t traceback_score;
  int32_t nmatches;
  int32_t nmismatches;
  int32_t nopens;
  int32_t nindels;
  int32_t dynprogindex;
  int32_t new_leftgenomepos;
  int32_t new_rightgenomepos;
  int32_t exonhead;
  int32_t introntype;
  int32_t gap_index;
  int32_t gap_queryjump;
  double left_prob;
  double right_prob;
} gmapdp_genome_result;

/* Splice-site model of a probability-array entry */
#define GMAPDP_MAXENT_DONOR        0  /* Maxent_hr_donor_prob */
#define GMAPDP_MAXENT_ACCEPTOR     1  /* Maxent_hr_acceptor_prob */
#define GMAPDP_MAXENT_ANTIDONOR    2  /* Maxent_hr_antidonor_prob */
#define GMAPDP_MAXENT_ANTIACCEPTOR 3  /* Maxent_hr_antiacceptor_prob */

/* Device MaxEnt.  The engine evaluates Maxent_hr_{donor,acceptor,antidonor,antiacceptor}_prob
 * (maxent_hr.c:27357 / 27433 / 27512 / 27586) itself, on the HBM-resident genome, bit-identical doubles
 * (genomealt == genome, the engine's scope).  The model tables are the reference's constants
 * (maxent_hr.c:25-24660) as tools/make_maxent_tables.py writes them: maxent_hr_tables.bin next to
 * libgmapdp.so, or the file GMAPDP_MAXENT_TABLES names; loaded on first use, once per device.
 *   - genome gaps: pass splice_probs = NULL (gmapdp_genome_gap_batch[_known], gmapdp_dynprog_batch,
 *     gmapdp_mixed.splice_probs) and the probability entries are computed on the device in the batch's
 *     stream (nprobs / nsplice_probs still give the arena size, gmapdp_genome_prob_entries);
 *   - microexons: gmapdp_microexon_finish with cand_probs = NULL (gmapdp_mixed.finish_probs = NULL)
 *     evaluates the candidates' two sites in the finish kernel; gmapdp_mixed's "whole microexon" section
 *     runs search and finish in the one round trip;
 *   - plans: gmapdp_plan_bind_genome_maxent; gmapdp_microexon_plan_run with d_cand_probs = NULL.
 * Missing tables make these calls fail with GMAPDP_EINVAL ("maxent tables: ...") -- never a host
 * fallback. */
/* 1 when the tables load (host only, no device needed), else 0; path: the file used or looked for. */
int gmapdp_maxent_available (char *path, size_t path_bytes);
/* out[i] = Maxent_hr_<models[i]>_prob(splice_pos = positions[i], chroffset = chroffsets[i]) on ctx's genome
 * (synchronous). */
int gmapdp_maxent_sites (gmapdp_ctx *ctx, const gmapdp_coord_t *positions, const uint8_t *models,
                         const gmapdp_coord_t *chroffsets, size_t n, double *out);

/* Diagnostic: out[i] = 1 when the cross-species stage 2 (GMAPDP_S2_CANONICAL_MIDDLE) finds the link between
 * the seed ends prevpos[i] and currpos[i] canonical, else 0 -- the decision of stage2.c:1257-1312 alone, on
 * the universal coordinates it computes there (plus strand: prevpos < currpos; minus: currpos < prevpos),
 * over ctx's genome with chroffset as the MaxEnt calls' chromosome offset (synchronous).  chrhigh is the
 * sweep's other chromosome bound; the coordinates given already carry it. */
int gmapdp_canonical_links (gmapdp_ctx *ctx, const gmapdp_coord_t *prevpos, const gmapdp_coord_t *currpos, size_t n,
                            int plusp, gmapdp_coord_t chroffset, gmapdp_coord_t chrhigh, uint8_t *out);

/* Test / measurement aid: what the cross-species sweeps of ctx's device did since the last call (then cleared;
 * synchronises the device).  out8[0..4]: range-2 candidates tested in the walk of
 * score_querypos_lookback_one, by form of the evaluation -- the one-hit scalar form, the 64-lane chunks, the
 * prefetched one-hit form, the one-step window of one-hit entries, the one-step window of entries with several
 * hits; out8[5..6]: candidates tested from score_querypos_lookback_mult, scalar form and chunks; out8[7]: shifts
 * at which both dinucleotides matched and the two MaxEnt models were evaluated. */
int gmapdp_debug_canon_counters (gmapdp_ctx *ctx, unsigned long long *out8);

/* For each problem, write glengthL + glengthR (splicesitepos, model) pairs
 * at the problem's prob_offset: the arguments of the Maxent_hr_*_prob call
 * (with the problem's chroffset) whose result belongs at that entry
 * (dynprog_genome.c:2573-2660).  Host-only; no device needed. */
int gmapdp_genome_splice_sites (const gmapdp_genome_problem *problems, int n, gmapdp_coord_t *positions,
                                uint8_t *models, size_t nentries);
/* Entries of the probability arena needed by the batch (max prob_offset + glengthL + glengthR). */
size_t gmapdp_genome_prob_entries (const gmapdp_genome_problem *problems, int n);

/* Run n Dynprog_genome_gap problems (same conventions as the other batches).
 * splice_probs: host arena of gmapdp_genome_prob_entries doubles. */
int gmapdp_genome_gap_batch (gmapdp_ctx *ctx, const gmapdp_genome_problem *problems, int n,
                             const char *qseq, const char *qseq_uc, size_t qbytes,
                             const double *splice_probs, size_t nprobs,
                             gmapdp_genome_result *results, gmapdp_pair *pairs, size_t pair_capacity);
/* The same with the known-site arena (nknown bytes) of GMAPDP_KNOWN_SITES problems. */
int gmapdp_genome_gap_batch_known (gmapdp_ctx *ctx, const gmapdp_genome_problem *problems, int n,
                                   const char *qseq, const char *qseq_uc, size_t qbytes,
                                   const double *splice_probs, size_t nprobs, const uint8_t *known_sites,
                                   size_t nknown, gmapdp_genome_result *results, gmapdp_pair *pairs,
                                   size_t pair_capacity);
/* Bytes of the problem's region of the known-site arena: glengthL + glengthR + 2 * (rlength + 1). */
size_t gmapdp_genome_known_bytes (const gmapdp_genome_problem *problem);
size_t gmapdp_genome_pair_capacity (const gmapdp_genome_problem *problems, int n);

/* Dynprog_single_gap + Dynprog_end5/3_gap + Dynprog_genome_gap calls of many callers in one
 * synchronous batch (the drop-in's dispatcher: one launch set for whatever GMAP's worker threads have
 * issued meanwhile).  One query arena (all qoff index qseq / qseq_uc), one splice-probability arena;
 * results has nsingle + nend entries (singles first), genome_results ngenome; pair_capacity at least
 * gmapdp_single_pair_capacity + gmapdp_end_pair_capacity + gmapdp_genome_pair_capacity. */
int gmapdp_dynprog_batch (gmapdp_ctx *ctx, const gmapdp_single_problem *singles, int nsingle,
                          const gmapdp_end_problem *ends, int nend, const gmapdp_genome_problem *genomes, int ngenome,
                          const char *qseq, const char *qseq_uc, size_t qbytes, const double *splice_probs,
                          size_t nprobs, gmapdp_result *results, gmapdp_genome_result *genome_results,
                          gmapdp_pair *pairs, size_t pair_capacity);

/* One Dynprog_cdna_gap call (dynprog_cdna.c:787 argument list): a cDNA insertion between two
 * anchors.  rsequenceL / rsequence_ucL = qseq / qseq_uc + qoffL (the L piece's first character),
 * rev_rsequenceR / rev_rsequence_ucR = qseq / qseq_uc + qoffR (the R piece's LAST character).  The
 * SHORTGAP block pushed when the bridge leaves a 9 x 9 gap reads rsequenceL up to
 * rev_roffsetR - roffsetL, so the arena must hold qseq[qoffL .. qoffL + rev_roffsetR - roffsetL].
 * Penalties are CDNA_OPEN/CDNA_EXTEND (dynprog_cdna.c:32-38) whatever the mode.
 * Domain: rlengthL == rlengthR >= glength, as stage3.c passes (both pieces queryjump' = genomejump +
 * extramaterial_paired, stage3.c:9275); outside it the reference's bridge reads cells no fill wrote,
 * and the engine rejects the batch with GMAPDP_EINVAL. */
typedef struct {
  int32_t qoffL;
  int32_t qoffR;
  int32_t rlengthL;
  int32_t rlengthR;
  int32_t glength;
  int32_t roffsetL;
  int32_t rev_roffsetR;
  int32_t goffset;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t flags;          /* GMAPDP_WATSON | GMAPDP_JUMP_LATE | GMAPDP_SIMD */
  int32_t genestrand;
  int32_t extraband;      /* extraband_paired */
  int32_t dynprogindex;
  double defect_rate;
} gmapdp_cdna_problem;

/* Out-parameters of Dynprog_cdna_gap.  traceback_score is GMAPDP_UNSET where the reference leaves
 * it unwritten (the glength <= 1 and size-guard NULL returns).  When the bridge leaves anything but
 * a 9 x 9 block, the list carries a gap holder (Pairpool_push_gapholder, dynprog_cdna.c:1270) at
 * pairs[gap_index] with jump = genomejump and incompletep = 1. */
typedef struct {
  int32_t npairs;          /* 0 <=> NULL List_T */
  int32_t pair_offset;
  int32_t traceback_score;
  int32_t dynprogindex;
  int32_t incompletep;
  int32_t gap_index;       /* -1: no gap holder */
  int32_t gap_queryjump;
  int32_t pad_;
} gmapdp_cdna_result;

int gmapdp_cdna_gap_batch (gmapdp_ctx *ctx, const gmapdp_cdna_problem *problems, int n,
                           const char *qseq, const char *qseq_uc, size_t qbytes,
                           gmapdp_cdna_result *results, gmapdp_pair *pairs, size_t pair_capacity);
size_t gmapdp_cdna_pair_capacity (const gmapdp_cdna_problem *problems, int n);

/* One Dynprog_end5_splicejunction (end3p = 0, dynprog_end.c:1653) or Dynprog_end3_splicejunction
 * (end3p = 1, dynprog_end.c:2249) call: the known-splice-site end alignment Splicetrie_solve_end5/3
 * (splicetrie.c) run for each candidate far exon.  The query slice is qseq[qoff .. qoff+rlength) as
 * for an end-gap problem: end5's rev_rsequence points at its LAST character.  The junction string
 * (the caller's splicejunction buffer, built by Dynprog_make_splicejunction_5/3) is
 * jseq[joff .. joff+glength) in string order: end5's rev_gsequence points at its last character,
 * end3's gsequence at its first.  Junction characters must be A C G T or N.  Nosimd semantics
 * (Dynprog_standard + traceback_local_std), or with GMAPDP_SIMD the SIMD builds' (the
 * Dynprog_simd_8/16_upper/_lower triangles + traceback_local_8/16_upper/_lower; rlength > glength + 1
 * is then GMAPDP_EINVAL, as for the SIMD end gaps). */
typedef struct {
  int32_t qoff;
  int32_t joff;
  int32_t rlength;
  int32_t glength;
  int32_t roffset;          /* (rev_)roffset */
  int32_t goffset_anchor;   /* (rev_)goffset_anchor */
  int32_t goffset_far;      /* (rev_)goffset_far */
  int32_t contlength;
  int32_t flags;            /* GMAPDP_JUMP_LATE */
  int32_t genestrand;
  int32_t extraband;        /* extraband_end */
  int32_t end3p;
  int32_t dynprogindex;
  int32_t pad_;
  double defect_rate;
} gmapdp_sj_problem;

/* Out-parameters of the splice-junction end gaps.  NULL (npairs 0) with the size guard's values
 * (traceback_score 0, missscore -100, counters 0) for lengths outside 1..660 x 1..2000; NULL with
 * everything but dynprogindex GMAPDP_UNSET when the best endpoint scores below 0 (the reference
 * writes nothing then).  Otherwise the list's pairs[known_index] is the known-splice gap holder
 * (Pairpool_push_gapholder with knownp = true, jump = its genomejump). */
typedef struct {
  int32_t npairs;
  int32_t pair_offset;
  int32_t traceback_score;
  int32_t missscore;
  int32_t nmatches;
  int32_t nmismatches;
  int32_t nopens;
  int32_t nindels;
  int32_t dynprogindex;
  int32_t known_index;      /* -1 for NULL */
} gmapdp_sj_result;

int gmapdp_end_splicejunction_batch (gmapdp_ctx *ctx, const gmapdp_sj_problem *problems, int n,
                                     const char *qseq, const char *qseq_uc, size_t qbytes,
                                     const char *jseq, size_t jbytes,
                                     gmapdp_sj_result *results, gmapdp_pair *pairs, size_t pair_capacity);
size_t gmapdp_sj_pair_capacity (const gmapdp_sj_problem *problems, int n);

/* Dynprog_microexon_int (dynprog_single.c:900, replaced at stage3.c:9664): the
 * microexon search inside an intron, in two steps because the reference scores each candidate with the
 * host's MaxEnt model (Maxent_hr_*_prob, maxent_hr.c:27357-27600) between finding and choosing:
 *   1. gmapdp_microexon_search lists each problem's candidates in the reference's loop order (cL
 *      ascending, cR ascending, occurrences as BoyerMoore_nt lists them: descending), with the two
 *      splice sites (position, GMAPDP_MAXENT_* model) whose probabilities prob2 / prob3 it needs;
 *   2. the caller evaluates them (candidate k's prob2 at cand_probs[2 (cand_offset + k)], prob3 next);
 *   3. gmapdp_microexon_finish keeps the first candidate whose (float) prob2 + prob3 beats the best so
 *      far and emits make_microexon_pairs_double's list (dynprog_single.c:683): left piece, gap holder,
 *      microexon, gap holder, right piece.  The gap holders carry comp = '>' (cdna_direction > 0) or
 *      '<' and jump = genomejump; queryjump is 0.
 * rsequence = qseq + qoff (queryseq + roffset as stage3.c passes it); results[i].pair_offset is
 * problem i's slot in the pair arena (rlength + 2 records, gmapdp_microexon_pair_capacity). */
typedef struct {
  int32_t qoff;
  int32_t rlength;
  int32_t roffset;
  int32_t goffsetL;
  int32_t rev_goffsetR;
  int32_t cdna_direction;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t watsonp;
  int32_t genestrand;
  int32_t dynprogindex;
  int32_t pad_;
} gmapdp_microexon_problem;

typedef struct {
  int32_t cL, cR;          /* lengths of the left and right pieces */
  int32_t candidate;       /* genomic offset of the microexon (goffsetM) */
  int32_t middlelength;
  gmapdp_coord_t pos2, pos3;  /* splice_pos of prob2 and prob3 (universal coordinates) */
  int32_t model2, model3;  /* GMAPDP_MAXENT_* */
} gmapdp_microexon_candidate;

typedef struct {
  int32_t ncandidates;
  int32_t dynprogindex;    /* after the call */
  int32_t microintrontype; /* intron.h: GTAG_FWD 0x20, GTAG_REV 0x04, NONINTRON 0 */
  int32_t npairs;          /* -1: NULL List_T */
  int64_t cand_offset;     /* first candidate in the candidate array */
  int64_t pair_offset;
  double bestprob2, bestprob3;
} gmapdp_microexon_result;

/* Step 1.  On GMAPDP_ESPACE (cand_capacity too small) *cands_needed holds the size required. */
int gmapdp_microexon_search (gmapdp_ctx *ctx, const gmapdp_microexon_problem *problems, int n,
                             const char *qseq, const char *qseq_uc, size_t qbytes, gmapdp_microexon_result *results,
                             gmapdp_microexon_candidate *candidates, size_t cand_capacity, size_t *cands_needed);
/* Step 3: results and candidates as step 1 left them; cand_probs as above. */
int gmapdp_microexon_finish (gmapdp_ctx *ctx, const gmapdp_microexon_problem *problems, int n,
                             const char *qseq, const char *qseq_uc, size_t qbytes,
                             const gmapdp_microexon_candidate *candidates, const double *cand_probs, size_t ncands,
                             gmapdp_microexon_result *results, gmapdp_pair *pairs, size_t pair_capacity);
size_t gmapdp_microexon_pair_capacity (const gmapdp_microexon_problem *problems, int n);

/* The GMAP drop-in's dispatcher batch in ONE round trip: gmapdp_dynprog_batch's calls,
 * gmapdp_microexon_search's calls and gmapdp_microexon_finish's calls (of other, earlier searches)
 * over one query arena -- one host-to-device copy, the kernels on the context's stream, one
 * device-to-host copy, one wait.  Each section means what the separate entry point's arguments
 * mean; a section with n = 0 is skipped.  The rare search that overflows the candidate pool is
 * rerun as gmapdp_microexon_search would (extra round trips).  GMAPDP_ESPACE: candidate_capacity too
 * small (*candidates_needed holds the size required); everything else is then still filled in.  Pair
 * arenas (pair_capacity, finish_pair_capacity, whole_pair_capacity) are checked up front against
 * gmapdp_*_pair_capacity of their calls: too small is GMAPDP_EINVAL, nothing run.  splice_probs = NULL / finish_probs = NULL: device MaxEnt (see "Device MaxEnt"). */
typedef struct {
  const gmapdp_single_problem *singles; int nsingle;
  const gmapdp_end_problem *ends; int nend;
  const gmapdp_genome_problem *genomes; int ngenome;
  const double *splice_probs; size_t nprobs;
  gmapdp_result *results;                    /* nsingle + nend */
  gmapdp_genome_result *genome_results;      /* ngenome */
  gmapdp_pair *pairs; size_t pair_capacity;
  const gmapdp_microexon_problem *searches; int nsearch;
  gmapdp_microexon_result *search_results;   /* nsearch */
  gmapdp_microexon_candidate *candidates; size_t candidate_capacity; size_t candidates_needed;
  const gmapdp_microexon_problem *finishes; int nfinish;
  const gmapdp_microexon_candidate *finish_candidates; const double *finish_probs; size_t nfinish_candidates;
  gmapdp_microexon_result *finish_results;   /* in: the searches' results; out: the choices */
  gmapdp_pair *finish_pairs; size_t finish_pair_capacity;
  const uint8_t *known_sites; size_t nknown; /* GMAPDP_KNOWN_SITES genome gaps' arena (else NULL, 0) */
  /* whole Dynprog_microexon_int calls: the search, the candidates' MaxEnt on the device and the choice,
   * all in this batch (the candidates stay on the device); whole_results as gmapdp_microexon_finish
   * leaves them, call i's pairs at the prefix sum of the earlier calls' rlength + 2
   * (gmapdp_microexon_pair_capacity) */
  const gmapdp_microexon_problem *wholes; int nwhole;
  gmapdp_microexon_result *whole_results;
  gmapdp_pair *whole_pairs; size_t whole_pair_capacity;
} gmapdp_mixed;
int gmapdp_mixed_batch (gmapdp_ctx *ctx, const char *qseq, const char *qseq_uc, size_t qbytes, gmapdp_mixed *m);

/* Device-resident microexon plan (the bench's path): descriptors uploaded once; the search is run at
 * plan time to size each call's candidate region, so gmapdp_microexon_plan_run writes candidates to
 * fixed regions (call i's at the prefix sum of the earlier calls' counts, device array
 * gmapdp_microexon_plan_device_candidates) and d_cand_probs (2 doubles per candidate, that order)
 * lines up with them.  what: 1 search, 2 finish, 3 both; qoff index the device arenas d_qseq /
 * d_qseq_uc; d_results (n records) and d_pairs (gmapdp_microexon_plan_pair_capacity records, call i's
 * at the prefix sum of rlength + 2) are the caller's device buffers. */
typedef struct gmapdp_microexon_plan gmapdp_microexon_plan;
int gmapdp_microexon_plan_create (gmapdp_ctx *ctx, const gmapdp_microexon_problem *problems, int n,
                                  const char *qseq, const char *qseq_uc, size_t qbytes,
                                  gmapdp_microexon_plan **plan);
size_t gmapdp_microexon_plan_candidates (const gmapdp_microexon_plan *plan);
size_t gmapdp_microexon_plan_pair_capacity (const gmapdp_microexon_plan *plan);
const gmapdp_microexon_candidate *gmapdp_microexon_plan_device_candidates (const gmapdp_microexon_plan *plan);
int gmapdp_microexon_plan_run (gmapdp_ctx *ctx, const gmapdp_microexon_plan *plan, const char *d_qseq,
                               const char *d_qseq_uc, const double *d_cand_probs, gmapdp_microexon_result *d_results,
                               gmapdp_pair *d_pairs, int what, void *stream);
void gmapdp_microexon_plan_destroy (gmapdp_microexon_plan *plan);

/* Stage-2 seeding: Oligoindex_hr_tally + Oligoindex_get_mappings
 * (oligoindex_hr.c:33849/34127) as Stage2_compute runs them for GMAP (stage2.c:6413-6501: one
 * 8-mer oligoindex, coveredp all false).  One problem = one (query, genomic window) pair:
 * queryuc_ptr = qseq_uc + qoff (upper-case query), the window [chrstart, chrend) of the chromosome
 * at chroffset..chrhigh on the plus (plusp) or minus strand.  minor selects
 * Oligoindex_array_new_minor's index (diag_lookback 60, suffnconsecutive 10) instead of the major
 * one (120, 20).  Domain: querylength > 8 (Oligoindex_set_inquery leaves stale state below that)
 * and at most 16384 distinct query 8-mers (a random sequence reaches that at about 18.9 kb).  A context
 * created with GMAPDP_CTX_LONG_QUERIES takes any query: one with more than 16384 distinct 8-mers (up to
 * all 65536) seeds in the "long" launch class, whose per-8-mer tables live in global memory, with the same
 * results; every stage-2 entry point accepts it, and a batch may mix short and long problems.
 * The context's mode (gmapdp_create) is the tally's: STANDARD, or a stranded cmet / atoi / ttoc mode
 * (Mode_T 1, 3, 5), in which the window's genome words are reduced before the 8-mers are taken
 * (count / store_positions_{fwd,rev}_std, oligoindex_hr.c:19293 / :30795; the query is not reduced).
 * In a context of a non-stranded mode (2, 4, 6: GMAP itself refuses them) every stage-2 entry point
 * -- this batch, gmapdp_stage2_batch and both plans -- returns GMAPDP_EINVAL.  A plan runs only on a
 * context of the mode of the one that made it. */
typedef struct {
  int32_t qoff;
  int32_t querylength;
  uint32_t chrstart;
  uint32_t chrend;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t plusp;
  int32_t minor;
} gmapdp_oligo_problem;

/* Per problem: *totalpositions, *maxnconsecutive, *oned_matrix_p (0 where the reference leaves it
 * unwritten: chrend <= chrstart) and the diagonals list (Diagpool_push records, list order) at
 * diagonals[4 * diag_offset ...]: {diagonal, querystart, queryend, nconsecutive} each.  Per query
 * position q: npositions[qoff + q] (0 without a full 8-mer or without hits) and
 * mappings[qoff + q], the index in `positions` of mappings[q][0] (-1 without hits); the problem's
 * table occupies positions[table_offset ...].  The batch's table arena stays below 2^31 entries
 * (GMAPDP_EINVAL otherwise; split the batch). */
typedef struct {
  int32_t totalpositions;
  int32_t maxnconsecutive;
  int32_t oned_matrix_p;
  int32_t ndiagonals;
  int64_t table_offset;
  int64_t diag_offset;
} gmapdp_oligo_result;

/* npositions, mappings: qbytes entries each (indexed like the query arena); mappings are absolute
 * indexes into `positions`.  Each problem writes its own query slice [qoff, qoff + querylength), so the
 * problems' slices must be disjoint (GMAPDP_EINVAL otherwise). */
int gmapdp_oligo_mappings_batch (gmapdp_ctx *ctx, const gmapdp_oligo_problem *problems, int n,
                                 const char *qseq_uc, size_t qbytes, gmapdp_oligo_result *results,
                                 int32_t *npositions, int32_t *mappings, uint32_t *positions,
                                 size_t positions_capacity, int32_t *diagonals, size_t diagonal_capacity);
/* Table entries / diagonal records (4 x int32) a batch may need. */
size_t gmapdp_oligo_positions_capacity (const gmapdp_oligo_problem *problems, int n);
size_t gmapdp_oligo_diagonal_capacity (const gmapdp_oligo_problem *problems, int n);
/* Device-resident path (bench / pipelined callers): plan once (distinct 8-mers, launch classes,
 * table / diagonal / scratch offsets; the descriptors are uploaded), then run asynchronously on
 * `stream` (hipStream_t; NULL = the context's stream) against a device-resident upper-case query
 * arena.  d_results has n entries in problem order; d_npositions / d_mappings are indexed like the
 * query arena, and a device mapping is relative to its problem's table: mappings[q][0] is
 * d_positions[table_offset + d_mappings[qoff + q]] (so the table arena may pass 2^31 entries);
 * d_positions / d_diagonals hold the plan's capacities.  A problem that needs more hit-list, table or
 * diagonal room than the layout gave it reports oned_matrix_p = -1 and writes nothing else. */
typedef struct gmapdp_oligo_plan gmapdp_oligo_plan;
int gmapdp_oligo_plan_create (gmapdp_ctx *ctx, const gmapdp_oligo_problem *problems, int n, const char *qseq_uc,
                              size_t qbytes, gmapdp_oligo_plan **plan);
size_t gmapdp_oligo_plan_positions_capacity (const gmapdp_oligo_plan *plan);
size_t gmapdp_oligo_plan_diagonal_capacity (const gmapdp_oligo_plan *plan);
int gmapdp_oligo_plan_nlaunches (const gmapdp_oligo_plan *plan);
int gmapdp_oligo_plan_run (gmapdp_ctx *ctx, const gmapdp_oligo_plan *plan, const char *d_qseq_uc,
                           gmapdp_oligo_result *d_results, int32_t *d_npositions, int32_t *d_mappings,
                           uint32_t *d_positions, int32_t *d_diagonals, void *stream);
void gmapdp_oligo_plan_destroy (gmapdp_oligo_plan *plan);

/* Stage2_scan (stage2.c:5610) as stage3_from_gregions calls it for every gregion before any
 * Stage2_compute (gmap.c:1855-1899): one seeding with the major 8-mer index (diag_lookback 120,
 * suffnconsecutive 20), coveredp all false, then Diag_update_coverage (diag.c:216).  A problem is a
 * gmapdp_oligo_problem whose fields are Stage2_scan's arguments (query slice, window, strand); minor must
 * be 0 (GMAPDP_EINVAL otherwise).  Domain and modes as for the seeding above: querylength > 8, STANDARD or
 * a stranded mode, GMAPDP_EINVAL in a context of mode 2, 4 or 6, GMAPDP_ENOGENOME without a genome.
 * Unlike gmapdp_oligo_mappings_batch, query slices may overlap or be identical (a read's gregions all point
 * at the same qoff): the seeding's per-position state lives in per-problem scratch.
 * chrend <= chrstart gives ncovered 0, stage2_source 1 (get_mappings returns before writing anything).
 * Only the results leave the device.  The batch runs as sub-batches, ordered on one stream, whose
 * worst-case scratch (table, diagonals, hit list, event pool, per-position arrays) fits a budget, so
 * memory does not grow with n.  The budget is the number of bytes the context's grow-only seeding buffers
 * hold when the plan is made, at least 8 GiB (~950 regions of a 2-kb read on a 214-kb gregion; a plan
 * allocates only what its largest sub-batch needs); GMAPDP_SCAN_ARENA_MB (read at plan creation) overrides
 * both; one problem alone always fits (the budget grows to its worst case).  The capacities are worst
 * cases, so a seeding layout overflow cannot happen; should one be reported all the same, the problem's
 * result is {-1, 0, totalpositions, 0} and the batch call returns GMAPDP_ELAUNCH with gmapdp_last_error
 * set -- never a plausible-looking count. */
typedef struct {
  int32_t ncovered;         /* Stage2_scan's return value */
  int32_t stage2_source;    /* *stage2_source: 1 (one 8-mer source) */
  int32_t totalpositions;   /* the seeding's, for diagnostics */
  int32_t maxnconsecutive;
} gmapdp_scan_result;

int gmapdp_stage2_scan_batch (gmapdp_ctx *ctx, const gmapdp_oligo_problem *problems, int n,
                              const char *qseq_uc, size_t qbytes, gmapdp_scan_result *results);
/* Device-resident form: plan once, then run asynchronously on `stream` (hipStream_t; NULL = the context's
 * stream) against a device-resident upper-case query arena laid out like the one the plan was made from.
 * d_results has n entries in problem order.  The plan owns its scratch, so its runs may overlap DP plans
 * on other streams; two runs of one plan must be ordered.  gmapdp_scan_plan_nlaunches: the sub-batches
 * of one run (three kernels each); _scratch_bytes: the device bytes the plan holds. */
typedef struct gmapdp_scan_plan gmapdp_scan_plan;
int gmapdp_scan_plan_create (gmapdp_ctx *ctx, const gmapdp_oligo_problem *problems, int n, const char *qseq_uc,
                             size_t qbytes, gmapdp_scan_plan **plan);
int gmapdp_scan_plan_run (gmapdp_ctx *ctx, const gmapdp_scan_plan *plan, const char *d_qseq_uc,
                          gmapdp_scan_result *d_results, void *stream);
int gmapdp_scan_plan_nlaunches (const gmapdp_scan_plan *plan);
size_t gmapdp_scan_plan_scratch_bytes (const gmapdp_scan_plan *plan);
void gmapdp_scan_plan_destroy (gmapdp_scan_plan *plan);

/* Stage2_compute (stage2.c:6325) as GMAP's update_stage3middle_list calls it (gmap.c:1208-1215):
 * query_offset 0, genestrand 0, proceed_pctcoverage 0.3, the major oligoindex array (8-mers,
 * diag_lookback 120, suffnconsecutive 20), localp, skip_repetitive_p, favor_right_p false,
 * max_nalignments 10; Stage2_setup (gmap.c:6544) without SNPs, cross-species canonical scoring
 * (gmap --cross-species) by `flags`, the context's mode (STANDARD or a stranded cmet / atoi / ttoc mode, see gmapdp_oligo_problem: there the
 * pairs' genome characters are the real genome's and comp is ':' where the query character differs,
 * convert_to_nucleotides stage2.c:5403-5452), sufflookback 60, nsufflookback 5.  queryseq_ptr = qseq + qoff
 * (case as given, the Pair cdna), queryuc_ptr = qseq_uc + qoff.  Domain as for gmapdp_oligo_problem: querylength > 8, and
 * genomic positions below 2^31 (Pairpool_push drops negative ones; the engine does not model that). */
typedef struct {
  int32_t qoff;
  int32_t querylength;
  uint32_t chrstart;
  uint32_t chrend;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t plusp;
  int32_t splicingp;       /* Stage2_setup's splicingp_in (novelsplicingp || knownsplicingp) */
  int32_t maxintronlen;    /* Stage2_setup's maxintronlen_in */
  int32_t flags;           /* GMAPDP_S2_* bits; 0: GMAP's default.  One value per batch or plan */
} gmapdp_stage2_problem;

/* gmapdp_stage2_problem.flags.  GMAPDP_S2_CANONICAL_MIDDLE: Stage2_setup's cross_species_p
 * (use_canonical_middle_p, stage2.c:139-143).  Range 2 of score_querypos_lookback_one / _mult
 * (stage2.c:1252-1321 / 1816-1881) then takes NON_CANONICAL_PENALTY_MIDDLE (4) off every candidate link
 * across a genomic skip unless Genome_sense_canonicalp or Genome_antisense_canonicalp
 * (genome_canonical.c:361 / 466) finds a GT..AG (CT..AC) pair at one shift in the two 23-nt windows
 * around the seed ends with both MaxEnt probabilities above 0.9 -- evaluated on the device over the
 * context's genome (genomealt == genome) with the device MaxEnt tables, in every stage-2 entry point
 * (gmapdp_stage2_batch, gmapdp_stage2_plan_create / _run / _fetch, the compact stream).  All calls of one
 * batch or plan carry the same flags: a mix, or a bit not listed here, is GMAPDP_EINVAL.  Without the
 * MaxEnt tables the flag fails with GMAPDP_EINVAL ("maxent tables: ..."), as device MaxEnt does for genome
 * gaps. */
#define GMAPDP_S2_CANONICAL_MIDDLE 1

/* Per call: the returned List_T of Stage2_T, in list order, as nresults path records starting at
 * paths[path_offset]; each record's pairs are its Stage2_middle list (all_starts / all_ends are NULL
 * in this build of the reference).  status: 0 no positions, 1 the coverage filter declined
 * (stage2.c:6526), 2 chained; negative: GMAPDP internal (never returned by gmapdp_stage2_batch). */
typedef struct {
  int32_t nresults;
  int32_t npaths;          /* paths traced before Stage2_filter_unique */
  int32_t ncovered;        /* Diag_update_coverage's ncovered */
  int32_t status;
  int32_t diag_querystart; /* Diag_compute_bounds' query bounds (status 2) */
  int32_t diag_queryend;
  int32_t path_offset;
  int32_t npairs;          /* pair records of all nresults paths */
} gmapdp_stage2_result;

typedef struct {
  int64_t pair_offset;     /* first record in the pair arena */
  int32_t npairs;
  int32_t pad_;
} gmapdp_path;

/* One Pair_T of a stage-2 path (convert_to_nucleotides): querypos, genomepos, cdna, comp ('|'; in a
 * stranded cmet / atoi / ttoc context ':' where the query differs from the genome), genome, genomealt; a gap holder (Pairpool_push_gapholder) has querypos = genomepos = -1, its
 * queryjump / genomejump, and blanks; ordinary pairs carry queryjump = genomejump = 0. */
typedef struct {
  int32_t querypos;
  int32_t genomepos;
  int32_t queryjump;
  int32_t genomejump;
  char cdna;
  char comp;
  char genome;
  char genomealt;
} gmapdp_path_pair;

#define GMAPDP_ESPACE (-6)  /* an output arena is too small: *_needed say how large it must be */

/* n Stage2_compute calls.  results: n entries.  paths / pairs: caller arenas of path_cap / pair_cap
 * records; on GMAPDP_ESPACE nothing else is valid and *paths_needed / *pairs_needed hold the sizes the
 * call needs (call again with larger arenas).  On success they hold the records used. */
int gmapdp_stage2_batch (gmapdp_ctx *ctx, const gmapdp_stage2_problem *problems, int n, const char *qseq,
                         const char *qseq_uc, size_t qbytes, gmapdp_stage2_result *results, gmapdp_path *paths,
                         size_t path_cap, gmapdp_path_pair *pairs, size_t pair_cap, size_t *paths_needed,
                         size_t *pairs_needed);

/* The three stage-2 entry points stage 3 calls on a segment of the query, with stage 3's arguments
 * (oligoindices_minor: 8-mers, diag_lookback 60, suffnconsecutive 10; skip_repetitive_p false, favor_right_p
 * false, genestrand 0, genomealt == genome, use_canonical_middle_p false; Stage2_setup as for
 * gmapdp_stage2_problem):
 *   GMAPDP_S2X_ONE   Stage2_compute_one (stage2.c:6754) as stage3.c:11382 calls it across a dual break: localp
 *                    true, middlep true, max_nalignments 1.  Zero or one list: the last path traced
 *                    (List_head(all_paths)), converted with gap holders, returned 3' end first
 *                    (List_reverse(middle)).
 *   GMAPDP_S2X_ENDS  Stage2_compute_ends (stage2.c:7087) as stage3.c:15849 / 16068 call it for an unaligned 3'
 *                    end: localp false, middlep false, max_nalignments 1.  A hit without a predecessor scores 0,
 *                    and a query position where no hit scored above 0 restarts all its hits at score 8
 *                    (stage2.c:3955-3980).  Every traced path is converted without gap holders (5' end first) and
 *                    the lists go through Stage2pairs_filter_unique_ends (:6218).
 *   GMAPDP_S2X_STARTS Stage2_compute_starts (stage2.c:6914) as stage3.c:15955 / 16166 call it for an unaligned 5'
 *                    end: ENDS' arguments with align_compute_lookforward (:5062).  The sweep runs from the last
 *                    query position down and links every hit to one further 3'; a path is traced from its cell
 *                    towards the 3' end, and MIN_TERMINAL_NCONSECUTIVE prunes its 5' end.  Every traced path
 *                    is converted without gap holders and returned 3' end first (List_reverse(pairs), :7040);
 *                    the lists go through Stage2pairs_filter_unique_starts (:6114: by the first pair's genomepos
 *                    descending, then the last pair's descending).
 * None applies the coverage filter (they chain whenever totalpositions > 0), all take Diag_max_bounds
 * (diag.c:894: every query position is active over the whole window, querystart 0, queryend querylength - 1)
 * and add query_offset to every pair's querypos.  The struct is gmapdp_stage2_problem followed by kind and
 * query_offset; flags must be 0 (cross-species scoring is not offered for these calls).  Domain as for
 * gmapdp_oligo_problem: querylength > 8 (chrend may equal chrstart or chrstart - 1, stage3.c:11379: no
 * positions), genomic positions below 2^31, the context's mode STANDARD or stranded. */
#define GMAPDP_S2X_ONE  1
#define GMAPDP_S2X_ENDS 2
#define GMAPDP_S2X_STARTS 3
typedef struct {
  int32_t qoff;
  int32_t querylength;
  uint32_t chrstart;
  uint32_t chrend;
  gmapdp_coord_t chroffset;
  gmapdp_coord_t chrhigh;
  int32_t plusp;
  int32_t splicingp;
  int32_t maxintronlen;
  int32_t flags;           /* must be 0 */
  int32_t kind;            /* GMAPDP_S2X_ONE, _ENDS or _STARTS; one value per batch */
  int32_t query_offset;    /* added to every pair's querypos (convert_to_nucleotides) */
} gmapdp_stage2x_problem;

/* n calls of one kind, in gmapdp_stage2_batch's formats: per call the returned lists in the returned list's
 * order (ONE: nresults 0 or 1) as path records, each record's pairs in that list's order (ONE and STARTS: 3' end
 * first).  status is 0 (no
 * positions) or 2 (chained), npaths the paths traced, diag_querystart / diag_queryend 0 / querylength - 1.
 * GMAPDP_ESPACE and *paths_needed / *pairs_needed as in gmapdp_stage2_batch.  GMAPDP_EINVAL (with a
 * message): a mix of kinds, a kind outside 1..3, flags != 0, querylength <= 8, a negative maxintronlen,
 * a context of a non-stranded cmet / atoi / ttoc mode (2, 4, 6).  GMAPDP_ENOGENOME without a genome. */
int gmapdp_stage2x_batch (gmapdp_ctx *ctx, const gmapdp_stage2x_problem *problems, int n, const char *qseq,
                          const char *qseq_uc, size_t qbytes, gmapdp_stage2_result *results, gmapdp_path *paths,
                          size_t path_cap, gmapdp_path_pair *pairs, size_t pair_cap, size_t *paths_needed,
                          size_t *pairs_needed);

/* Device-resident Stage2_compute (bench / pipelined callers): plan once (the seeding plan, the
 * chaining scratch sized from one seeding run at plan time, output pools), then run asynchronously on
 * `stream` against device-resident query arenas.  what: 1 seeding only, 2 chaining only (after a
 * seeding run), 3 both.  d_results: n entries in problem order; paths and pairs stay in the plan's
 * pools (gmapdp_stage2_plan_outputs: device pointers and the counters {scratch, paths, pairs} bytes /
 * records used); a result with status -2 did not fit them.
 * Split chaining: what = 4, 8 or 16 runs one chaining kernel alone (s2a with its two ordering passes, the
 * s2b sweep, s2c).  1, then 4, 8, 16 in that order (on one stream, or each ordered after the one before by
 * an event) is a supported way to run the chain and gives exactly what = 3 gives: results, pools and pool
 * counters (tests/test_gpu_bench_step.py; bench.py's timed step runs it so, on a plan that never made a
 * full run).  s2a needs the seeding of the same query arenas before it, s2b that s2a, s2c that s2b; the
 * pool counters restart with s2a and again with s2c, which alone appends to the pools.  One of them re-run
 * alone (profiling) works over the scratch the previous phases of the same query left.
 * In flight at once on one context: a stage-2 plan owns its seeding arenas, chaining scratch, pools and
 * counters, so its runs may overlap any DP or microexon plan's runs (tested: block k + 1's chain beside block
 * k's DP classes and microexon plan).  Runs of stage-2 plans are kept in order on one stream by bench.py and
 * the tests; two runs of the same plan must be ordered (they share all of the above), and so must a run and
 * a gmapdp_stage2_plan_fetch of the pools it writes.  A microexon plan likewise owns its candidate arena and
 * runs beside a DP plan's launches (tested); two runs of the same plan must be ordered.  DP plans: see
 * gmapdp_plan_run_launch.
 * Creating a plan of any kind sizes the context's grow-only buffers and runs on the context's stream:
 * create plans while no run is in flight on the context.
 * The pools are fixed when the plan is made (16 + 4 n path records, 64 + 3 * the sum of the query lengths pair
 * records) and never grow.  A call that does not fit reserves its slots all the same, in the order the waves
 * finish, and reports status -2: its result's other fields are not to be used.  Of its path slots, those below
 * the pool's capacity hold either a list it wrote before its pair reservation failed (a valid record, its pairs
 * in the pool, owned by no call a caller should read) or an empty record (pair_offset 0, npairs 0); none holds
 * uninitialised memory or an earlier run's record.  Its reserved pair slots are not written.  The counters
 * count past the capacities; gmapdp_stage2_plan_fetch clamps them, gmapdp_stage2_plan_compact_pairs takes a
 * count above the path pool's size as that size.  The lists of all path records within the pool are disjoint
 * and lie within the pair pool, so the compact stream keeps to gmapdp_stage2_plan_compact_bound whatever
 * overflowed. */
typedef struct gmapdp_stage2_plan gmapdp_stage2_plan;
int gmapdp_stage2_plan_create (gmapdp_ctx *ctx, const gmapdp_stage2_problem *problems, int n, const char *qseq,
                               const char *qseq_uc, size_t qbytes, gmapdp_stage2_plan **plan);
int gmapdp_stage2_plan_run (gmapdp_ctx *ctx, const gmapdp_stage2_plan *plan, const char *d_qseq,
                            const char *d_qseq_uc, gmapdp_stage2_result *d_results, int what, void *stream);
int gmapdp_stage2_plan_outputs (const gmapdp_stage2_plan *plan, gmapdp_path **d_paths, gmapdp_path_pair **d_pairs,
                                unsigned long long **d_counters, size_t *scratch_bytes);
/* The outputs of a finished gmapdp_stage2_plan_run (chaining) on `stream` (NULL = the context's stream;
 * synchronised here), in gmapdp_stage2_batch's format: n results copied from d_results, and the path
 * and pair records into host arenas of path_cap / pair_cap records (GMAPDP_ESPACE with *_needed when
 * they are too small).  A result with status -2 overflowed the plan's pools or its seeding layout. */
int gmapdp_stage2_plan_fetch (gmapdp_ctx *ctx, const gmapdp_stage2_plan *plan, const gmapdp_stage2_result *d_results,
                              void *stream, gmapdp_stage2_result *results, gmapdp_path *paths, size_t path_cap,
                              gmapdp_path_pair *pairs, size_t pair_cap, size_t *paths_needed, size_t *pairs_needed);
/* The seeding results of the plan's last run (n, problem order; table_offset / diag_offset index the plan's
 * own arenas), synchronising `stream` (NULL = the context's). */
int gmapdp_stage2_plan_seeding_results (gmapdp_ctx *ctx, const gmapdp_stage2_plan *plan, void *stream,
                                        gmapdp_oligo_result *out);
/* How many of the plan's calls seed with 16-bit and with 32-bit counters (after the plan's sizing run
 * moved every call with fewer than 2^16 hits to the 16-bit class).  Calls of the long class
 * (GMAPDP_CTX_LONG_QUERIES), whose counters are always 32-bit, are counted with n32. */
int gmapdp_stage2_plan_seeding_classes (const gmapdp_stage2_plan *plan, int *n16, int *n32);
/* Seeding problems the context has put into the long class so far, over all its stage-2 entry points
 * (0 for ever without GMAPDP_CTX_LONG_QUERIES). */
unsigned long long gmapdp_long_query_calls (const gmapdp_ctx *ctx);
/* How many times gmapdp_stage2_batch and gmapdp_stage2x_batch on this context have grown their device output
 * pools and run the chaining kernels again because a call reported an overflow (first guesses: 16 + 2 n path
 * records, 64 + 2 * the sum of the query lengths pair records; one count per extra attempt). */
unsigned long long gmapdp_stage2_pool_regrows (const gmapdp_ctx *ctx);
/* The compact stream of a finished chaining run's path pairs (gmapdp_plan_compact_pairs' format, 21-B RAW
 * ops: gmapdp_path_pair records with a jump or a negative position): one list per record of the plan's path
 * pool (*path_cap of them; records past the pool's count are empty lists).  d_offsets: path_cap + 1 uint64
 * (device), exclusive offsets and the total; d_out NULL sizes only, else at least
 * gmapdp_stage2_plan_compact_bound bytes (21 B per record of the pair pool, + 64).  gmapdp_expand_path_pairs
 * restores the records on the host, each path's npairs at its pair_offset of out's `capacity` records (the
 * path records as gmapdp_stage2_plan_fetch returns them); GMAPDP_EINVAL as gmapdp_expand_pairs. */
size_t gmapdp_stage2_plan_compact_bound (const gmapdp_stage2_plan *plan, size_t *path_cap);
int gmapdp_stage2_plan_compact_pairs (gmapdp_ctx *ctx, const gmapdp_stage2_plan *plan, uint8_t *d_out,
                                      uint64_t *d_offsets, void *stream);
int gmapdp_expand_path_pairs (const uint8_t *stream, const uint64_t *offsets, int npaths, const gmapdp_path *paths,
                              gmapdp_path_pair *out, size_t capacity, int nthreads);
/* The same over caller-made device buffers (gmapdp_stage2_plan_compact_pairs calls it with the plan's own):
 * path_cap gmapdp_path records of which the first *d_npaths count (the others, and a path with a negative
 * offset or count or with pair_offset + npairs > pair_cap, are empty lists); d_offsets: path_cap + 1 uint64;
 * d_out NULL sizes only, else at least gmapdp_compact_bound (pair_cap, 1) bytes, or the sizing pass's total. */
int gmapdp_compact_path_pairs (gmapdp_ctx *ctx, const gmapdp_path *d_paths, const uint64_t *d_npaths, size_t path_cap,
                               const gmapdp_path_pair *d_pairs, size_t pair_cap, uint8_t *d_out, uint64_t *d_offsets,
                               void *stream);
void gmapdp_stage2_plan_destroy (gmapdp_stage2_plan *plan);

/* Create a context on HIP device `device`.  mode = Mode_T (mode.h:5;
 * 0 = STANDARD, 1 / 3 / 5 the stranded cmet / atoi / ttoc modes, 2 / 4 / 6 the non-stranded ones: the
 * DP family in all seven, stage 2 in STANDARD and the stranded ones).  user_* mirror
 * Dynprog_single_setup. */
int gmapdp_create (gmapdp_ctx **ctx, int device, int mode,
                   int user_open, int user_extend, int user_dynprog_p);
void gmapdp_destroy (gmapdp_ctx *ctx);
/* gmapdp_create with flags, for callers that run several contexts at once (the GMAP drop-in's
 * dispatcher threads): GMAPDP_CTX_ONE_STREAM creates no side streams (a process has few hardware
 * queues, GPU_MAX_HW_QUEUES, and streams beyond them share one and serialise); GMAPDP_CTX_PRIO_HIGH /
 * _LOW create the context's stream at the device's highest / lowest priority; GMAPDP_CTX_BLOCKING_SYNC
 * makes the synchronous batch calls wait without spinning; GMAPDP_CTX_POLL_SYNC makes them poll the
 * batch's completion every GMAPDP_POLL_US microseconds (default 10) and sleep in between. */
#define GMAPDP_CTX_ONE_STREAM 0x1
#define GMAPDP_CTX_PRIO_HIGH  0x2
#define GMAPDP_CTX_PRIO_LOW   0x4
#define GMAPDP_CTX_BLOCKING_SYNC 0x8  /* batch calls sleep on a blocking-sync event instead of spinning */
#define GMAPDP_CTX_POLL_SYNC 0x10     /* batch calls poll their completion, sleeping between polls */
/* Plans spread their launch classes (longest-processing-time first) over the caller's stream and two
 * side streams instead of three: for a caller that keeps the process's fourth hardware queue for other
 * work of its own, e.g. Stage2_compute on its own stream beside the plan (bench.py), so that no stream
 * receives two of the plan's lists. */
#define GMAPDP_CTX_TWO_SIDES 0x20
/* Stage 2 takes queries with more than 16384 distinct 8-mers (gmapdp_oligo_problem's domain text); without
 * the flag every stage-2 entry point refuses them with GMAPDP_EINVAL.  Queries within the bound seed exactly
 * as without the flag. */
#define GMAPDP_CTX_LONG_QUERIES 0x40
int gmapdp_create_ex (gmapdp_ctx **ctx, int device, int mode, int user_open, int user_extend, int user_dynprog_p,
                      int flags);
/* Use `owner`'s HBM-resident genome in `ctx` (no copy; same device).  `owner` must outlive every
 * context sharing its genome and keep that genome until they are done. */
int gmapdp_share_genome (gmapdp_ctx *ctx, const gmapdp_ctx *owner);
/* A packed genome resident in one device's HBM, independent of any context: upload once, then let any
 * number of contexts read it (gmapdp_use_dgenome; no copy).  The drop-in keeps one per GMAP Genome_T
 * (a -g run over a multi-sequence file has several).  Destroy it only after every context using it is
 * done with it. */
/* Grow the context's staging and scratch buffers to `bytes` each (4x for the direction and chaining
 * scratch) now, so that a long-running caller does not grow them later: a buffer's growth frees the old
 * one, and hipFree waits for the whole device, stalling every context's streams.  what: GMAPDP_RESERVE_DP
 * (single / end / genome-gap batches), _AUX (microexon and cDNA-gap batches), _STAGE2 (Stage2_compute and
 * seeding batches). */
#define GMAPDP_RESERVE_DP     0x1
#define GMAPDP_RESERVE_AUX    0x2
#define GMAPDP_RESERVE_STAGE2 0x4
int gmapdp_reserve (gmapdp_ctx *ctx, size_t bytes, int what);
typedef struct gmapdp_dgenome gmapdp_dgenome;
int gmapdp_dgenome_create (int device, const uint32_t *blocks, size_t nwords, uint64_t length, gmapdp_dgenome **g);
void gmapdp_dgenome_destroy (gmapdp_dgenome *g);
int gmapdp_use_dgenome (gmapdp_ctx *ctx, const gmapdp_dgenome *g);

/* Words needed for a packed genome of `length` nt ((len+31)/32*3 + 4). */
size_t gmapdp_genome_words (uint64_t length);
/* Pack characters into .genomecomp blocks (A=0 C=1 G=2 T=3, 32 nt per
 * {high, low, flags} triple, non-ACGT flagged).  `blocks` must hold
 * gmapdp_genome_words(length) words. */
int gmapdp_pack_genome (const char *seq, uint64_t length, uint32_t *blocks);
/* Upload packed blocks (e.g. Genome_blocks(genome) of a loaded GMAP
 * genome) to HBM.  nwords as returned by gmapdp_genome_words.  Genomes of
 * 2^32 nt or more (gmapl, 64-bit Univcoord_T) are GMAPDP_EINVAL. */
int gmapdp_set_genome (gmapdp_ctx *ctx, const uint32_t *blocks, size_t nwords, uint64_t length);

/* The alternate-allele genome (GMAP run with --use-snps hands every Dynprog_* entry a second Genome_T,
 * genomealt).  `blocks`: gmapdp_pack_genome of the alternate sequence, or GMAP's Genome_blocks(genomealt);
 * position for position beside the primary genome, which must be bound already with the same `length` and
 * `nwords` (GMAPDP_ENOGENOME without one, GMAPDP_EINVAL when they differ).  The engine reads the alternate
 * genome's high / low words only: 'N' goes where the PRIMARY genome's flag bit is set, as in the reference
 * (uncompress_mmap_snps_subst, Genome_get_char).  blocks == NULL unbinds it.  Binding a new primary genome
 * (gmapdp_set_genome, gmapdp_use_dgenome, gmapdp_share_genome) drops the alternate one;
 * gmapdp_share_genome shares the owner's alternate genome as well.
 *
 * While an alternate genome is bound:
 *  - nosimd Dynprog_single_gap / Dynprog_end5_gap / Dynprog_end3_gap run under it, bit-exact to the
 *    reference's nosimd build: a cell scores the larger table entry of the two alleles, a pair is a match
 *    through either allele, else ambiguous when either is consistent, else a mismatch, and every
 *    gmapdp_pair carries genomealt.  Entry points: gmapdp_single_gap_batch, gmapdp_end_gap_batch,
 *    gmapdp_dynprog_batch with ngenome == 0, gmapdp_plan_create / _plan_single / _plan_create_all without
 *    genome gaps, and gmapdp_plan_run / _plan_run_launch on such plans.  Every problem takes the band
 *    layout's alternate-allele kernel, one wave each (no packed narrow class, no rows layout).
 *  - everything else is GMAPDP_EINVAL before any launch, with gmapdp_last_error naming the family:
 *    GMAPDP_SIMD single / end problems; genome gaps (gmapdp_genome_gap_batch, _batch_known,
 *    gmapdp_dynprog_batch and plans with genome gaps); gmapdp_cdna_gap_batch;
 *    gmapdp_end_splicejunction_batch; gmapdp_microexon_*; gmapdp_mixed_batch; gmapdp_maxent_sites;
 *    gmapdp_canonical_links; gmapdp_oligo_*, gmapdp_scan_plan_*, gmapdp_stage2_scan_batch,
 *    gmapdp_stage2_* and gmapdp_stage2x_batch.
 * A plan remembers whether it was made under an alternate genome: running it in a context whose binding
 * (bound or not) differs from then is GMAPDP_EINVAL.  A context without one behaves exactly as before. */
int gmapdp_set_genome_alt (gmapdp_ctx *ctx, const uint32_t *blocks, size_t nwords, uint64_t length);
/* The same from an HBM-resident genome, no copy (g == NULL unbinds). */
int gmapdp_use_dgenome_alt (gmapdp_ctx *ctx, const gmapdp_dgenome *g);
/* 1 when an alternate genome is bound, else 0. */
int gmapdp_has_genome_alt (const gmapdp_ctx *ctx);

/* Run n Dynprog_single_gap problems.  Host arrays in, host arrays out
 * (the engine stages them through pinned device buffers).  `pairs` must
 * have room for gmapdp_single_pair_capacity(problems, n) records; result
 * i's pairs are pairs[results[i].pair_offset .. +npairs). */
int gmapdp_single_gap_batch (gmapdp_ctx *ctx, const gmapdp_single_problem *problems, int n,
                             const char *qseq, const char *qseq_uc, size_t qbytes,
                             gmapdp_result *results, gmapdp_pair *pairs, size_t pair_capacity);
size_t gmapdp_single_pair_capacity (const gmapdp_single_problem *problems, int n);

/* Run n Dynprog_end5_gap / Dynprog_end3_gap problems (same conventions).
 * NULL results follow dynprog_end.c: traceback_score 0; dynprogindex is left
 * unchanged on the early returns (rlength <= 0, end5 goffset < 0,
 * glength <= 0) and advanced otherwise. */
int gmapdp_end_gap_batch (gmapdp_ctx *ctx, const gmapdp_end_problem *problems, int n,
                          const char *qseq, const char *qseq_uc, size_t qbytes,
                          gmapdp_result *results, gmapdp_pair *pairs, size_t pair_capacity);
size_t gmapdp_end_pair_capacity (const gmapdp_end_problem *problems, int n);

/* Device-resident path for pipelined callers and throughput measurement.
 * gmapdp_plan_single resolves penalties, bands and launch classes once on
 * the host (problems resolved on the host -- the size guard -- are written
 * to host_results immediately) and uploads the descriptors.  The upload
 * may still be in flight when the create call returns (the host goes on to
 * its next work); the plan's first run waits for it, so nothing changes for
 * the caller.  gmapdp_plan_run then launches asynchronously on `stream` (a hipStream_t;
 * NULL = the context's stream) against device-resident query arenas; GPU
 * results land in d_results[gmapdp_plan_dev_index(plan, i)] and pairs in
 * d_pairs (capacity gmapdp_plan_pair_capacity). */
typedef struct gmapdp_plan gmapdp_plan;
/* Mixed batch: host_results has nsingle + nend entries (singles first). */
int gmapdp_plan_create (gmapdp_ctx *ctx, const gmapdp_single_problem *singles, int nsingle,
                        const gmapdp_end_problem *ends, int nend, gmapdp_result *host_results,
                        gmapdp_plan **plan);
int gmapdp_plan_single (gmapdp_ctx *ctx, const gmapdp_single_problem *problems, int n,
                        gmapdp_result *host_results, gmapdp_plan **plan);
/* All three families: host_results has nsingle + nend entries, host_genome_results
 * ngenome entries.  Launch members number the problems singles, ends, genome gaps. */
int gmapdp_plan_create_all (gmapdp_ctx *ctx, const gmapdp_single_problem *singles, int nsingle,
                            const gmapdp_end_problem *ends, int nend, const gmapdp_genome_problem *genomes,
                            int ngenome, gmapdp_result *host_results, gmapdp_genome_result *host_genome_results,
                            gmapdp_plan **plan);
/* Device buffers of the genome-gap problems: the splice-probability arena and the
 * results (indexed by gmapdp_plan_genome_dev_index).  Required before running a plan
 * that has genome-gap problems on the GPU. */
int gmapdp_plan_bind_genome (gmapdp_plan *plan, const double *d_splice_probs, gmapdp_genome_result *d_genome_results);
/* The same with device MaxEnt: d_splice_probs (gmapdp_genome_prob_entries doubles) is scratch that each
 * genome-gap launch class fills for its own problems on its own stream before its fill kernel. */
int gmapdp_plan_bind_genome_maxent (gmapdp_ctx *ctx, gmapdp_plan *plan, double *d_splice_probs,
                                    gmapdp_genome_result *d_genome_results);
int gmapdp_plan_genome_gpu_problems (const gmapdp_plan *plan);
int gmapdp_plan_genome_dev_index (const gmapdp_plan *plan, int j);
/* 0: Dynprog_single_gap / end-gap kernel (one problem per wave), 1: Dynprog_genome_gap
 * kernel, 2: packed single/end-gap kernel (64/S narrow-band problems per wave; for these
 * gmapdp_plan_launch_info reports R = S and lds = the per-problem LDS slot), 3: SIMD-build
 * single gaps (sx), 4: SIMD-build end gaps (uxe), 5: SIMD-build genome gaps (uxg),
 * 7: single/end gaps whose band is wider than the query (lanes over query rows) */
int gmapdp_plan_launch_kind (const gmapdp_plan *plan, int li);
size_t gmapdp_plan_pair_capacity (const gmapdp_plan *plan);
int gmapdp_plan_gpu_problems (const gmapdp_plan *plan);
int gmapdp_plan_dev_index (const gmapdp_plan *plan, int i);
int gmapdp_plan_nlaunches (const gmapdp_plan *plan);
int gmapdp_plan_run (gmapdp_ctx *ctx, const gmapdp_plan *plan, const char *d_qseq, const char *d_qseq_uc,
                     gmapdp_result *d_results, gmapdp_pair *d_pairs, void *stream);
/* The compact pair stream (run-length ops plus one character code per record; the host expands
 * it into the same records -- Pair_T lists -- with gmapdp_expand_pairs).  After gmapdp_plan_run on `stream`:
 * each GPU problem's list (dev slots 0..gmapdp_plan_gpu_problems - 1, then the genome gaps' slots) becomes a
 * byte stream; d_offsets (gpu problems + genome gpu problems + 1 uint64, device) receives the exclusive
 * offsets and the total.  d_out NULL: the offsets only (to size a copy); else at least
 * gmapdp_plan_compact_bound bytes: 18 B per record of the pair arena (a record that starts a run and whose
 * characters need the escape takes 13 + 5 B), + 64.  Stream format: pc_kernel.hip. */
size_t gmapdp_plan_compact_bound (const gmapdp_plan *plan);
int gmapdp_plan_compact_pairs (gmapdp_ctx *ctx, const gmapdp_plan *plan, const gmapdp_result *d_results,
                               const gmapdp_pair *d_pairs, uint8_t *d_out, uint64_t *d_offsets, void *stream);
/* The same over caller-made device buffers (gmapdp_plan_compact_pairs calls it with the plan's own): n
 * gmapdp_result records then ng gmapdp_genome_result records, each a list of npairs (negative: none)
 * records at pair_offset of d_pairs; d_offsets: n + ng + 1 uint64.  gmapdp_compact_bound: the most bytes
 * the stream of nrecords records takes (18 B each, 21 B for path pairs, + 64). */
size_t gmapdp_compact_bound (size_t nrecords, int is_path_pairs);
int gmapdp_compact_pairs (gmapdp_ctx *ctx, const gmapdp_result *d_results, int n,
                          const gmapdp_genome_result *d_gresults, int ng, const gmapdp_pair *d_pairs,
                          uint8_t *d_out, uint64_t *d_offsets, void *stream);
/* Host: problem i's ops (stream[offsets[i], offsets[i + 1])) back to its npairs[i] records at
 * out[pair_offsets[i]], on nthreads host threads (0: the plan builders' default); out holds `capacity`
 * records.  GMAPDP_EINVAL when a problem's ops do not decode to exactly its records and bytes (nothing
 * outside its ops is read), when its offsets decrease, or when its records do not lie inside out
 * (pair_offsets[i] < 0 or pair_offsets[i] + npairs[i] > capacity); nothing outside out is written. */
int gmapdp_expand_pairs (const uint8_t *stream, const uint64_t *offsets, int n, const int32_t *npairs,
                         const int64_t *pair_offsets, gmapdp_pair *out, size_t capacity, int nthreads);
/* Per-launch-class access (one kernel launch per class; for profiling). */
int gmapdp_plan_launch_info (const gmapdp_plan *plan, int li, int *R, int *dirs_lds, int *count, size_t *lds);
/* Launch classes are spread over the caller's stream (0) and three side streams (1..3),
 * longest-processing-time first; launches are numbered in issue order.  is_tail: 1 if the
 * launch runs on a side stream. */
int gmapdp_plan_launch_stream (const gmapdp_plan *plan, int li);
int gmapdp_plan_launch_is_tail (const gmapdp_plan *plan, int li);
/* Original problem indices of launch li (count entries, launch order). */
int gmapdp_plan_launch_members (const gmapdp_plan *plan, int li, int *problem_indices);
/* The context's direction scratch (spilled direction planes, bridge candidates; one grow-only buffer per
 * context, the offsets into it baked into the plan) that launch li's members can touch: the byte range
 * [*offset, *offset + *bytes) around them, 0, 0 when the launch uses none; gmapdp_plan_scratch_bytes is the
 * plan's total.  A problem's region follows the problems before it in problem order, not in launch order, so
 * the ranges of two launches usually interleave; what keeps launches apart is that their members' regions
 * are disjoint: gmapdp_plan_launch_member_scratch gives each member's own region (count entries, launch
 * order; 0, 0 for a member without scratch; a packed class -- kinds 2 and 3 -- has one region for the whole
 * launch, reported at its first member).  Read-only: sizes are recomputed from the descriptors. */
int gmapdp_plan_launch_scratch (const gmapdp_plan *plan, int li, uint64_t *offset, uint64_t *bytes);
int gmapdp_plan_launch_member_scratch (const gmapdp_plan *plan, int li, uint64_t *offsets, uint64_t *bytes,
                                       uint64_t *offset, uint64_t *total_bytes);
size_t gmapdp_plan_scratch_bytes (const gmapdp_plan *plan);
/* One launch on the caller's `stream` (gmapdp_plan_launch_stream names which of the caller's main and side
 * streams the plan's schedule means it for; the caller forks the side streams from main and joins them
 * back, as gmapdp_plan_run does with the context's own).  On one context:
 *   - the launches of ONE plan may all be in flight at once, on any streams: their members' scratch regions,
 *     result slots and pair ranges are disjoint, and a genome-gap class's MaxEnt prologue fills only its own
 *     members' entries of the bound probability arena (it must precede that class's kernel on its stream);
 *   - TWO DP plans (or two runs of one plan) must not be in flight together: every plan's regions start at
 *     byte 0 of the same scratch.  Order them on a stream (bench.py: every block's launches are forked from
 *     and joined into one stream);
 *   - stage-2 and microexon plans' runs share nothing with it and may overlap it (see
 *     gmapdp_stage2_plan_run);
 *   - the scratch only grows, and gmapdp_plan_create* already grows it to what the plan needs, so a run never
 *     does: plans of different sizes run in any order on one context.  Growing frees the old buffer, which
 *     waits for the whole device, so create plans while no run is in flight on the context.
 * tests/test_gpu_bench_step.py runs exactly this schedule against the oracle. */
int gmapdp_plan_run_launch (gmapdp_ctx *ctx, const gmapdp_plan *plan, int li, const char *d_qseq,
                            const char *d_qseq_uc, gmapdp_result *d_results, gmapdp_pair *d_pairs, void *stream);
/* The same launch's kernel alone: a genome-gap class's device-MaxEnt prologue is not re-run (the splice
 * probabilities a previous full run computed stay in the bound arena).  For timing one kernel's launches. */
int gmapdp_plan_run_launch_kernel (gmapdp_ctx *ctx, const gmapdp_plan *plan, int li, const char *d_qseq,
                                   const char *d_qseq_uc, gmapdp_result *d_results, gmapdp_pair *d_pairs,
                                   void *stream);
void gmapdp_plan_destroy (gmapdp_plan *plan);
/* The context's HIP stream (hipStream_t). */
void *gmapdp_stream (gmapdp_ctx *ctx);

void gmapdp_compute_bands (int *lband, int *uband, int rlength, int glength, int extraband, int widebandp);

/* Last error message for this context (static storage). */
const char *gmapdp_last_error (gmapdp_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
