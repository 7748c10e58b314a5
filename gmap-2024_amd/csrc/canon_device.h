// canon_device.h -- device restatement of the canonical-link test of GMAP's cross-species stage 2
// (gmap --cross-species: Stage2_setup's use_canonical_middle_p, stage2.c:139-143): the decision range 2 of
// score_querypos_lookback_one / _mult takes for every candidate link (stage2.c:1257-1312 / 1820-1871),
// Genome_sense_canonicalp then Genome_antisense_canonicalp (genome_canonical.c:361 / 466) over
// prev_dinucleotide_position (:210).
//
// The reference walks the donor dinucleotides and the acceptor dinucleotides of two 23-position windows
// downwards and merges the two walks by shift (right bound minus site): it answers true at the first shift
// where both windows hold their dinucleotide and both MaxEnt probabilities exceed 0.9, and false when
// either walk runs out -- an intersection by shift.  Here one lane takes one link and loops over the 23
// shifts; the models are evaluated only where both dinucleotides match (maxent_prob, me_device.h: the
// reference's doubles).
//
// With L < H the two seed ends (plus strand: L = prevpos, H = currpos; minus: L = currpos, H = prevpos),
// up = MISS_BEHIND 16 on the plus strand and GREEDY_ADVANCE 6 on the minus strand (the right bounds are
// pos + up, the left bounds pos + up - 22), rL = L + up, rH = H + up, and shift k = 0 .. 22:
//   sense      GT at (rL - k, rL - k + 1), AG at (rH - k - 2, rH - k - 1),
//              donor_prob(rL - k) > 0.9 and acceptor_prob(rH - k) > 0.9
//   antisense  AC at (rH - k - 2, rH - k - 1), CT at (rL - k, rL - k + 1),
//              antidonor_prob(rH - k) > 0.9 and antiacceptor_prob(rL - k) > 0.9
// so both tests read the same two 24-nt windows, [rL - 22, rL + 1] and [rH - 24, rH - 1] (inclusive).
// Early out (no site): L or H below GREEDY_ADVANCE (plus) / MISS_BEHIND (minus).  A flagged position (N,
// and anything past the genome's words) never matches (block_find clears both dinucleotides it touches);
// a dinucleotide straddling two 32-nt blocks matches like any other (high_halfsite & prev_low_halfsite).
// H may be 16 or 17 on the minus strand, where the reference's unsigned acceptor_leftbound - 2 wraps and it
// reads in front of the genome: here positions below 0 hold no site.
#pragma once
#include <stdint.h>

#include "me_device.h"

namespace gmapdp {

constexpr int kCanonGreedyAdvance = 6, kCanonMissBehind = 16;  // stage2.c:62-63
constexpr int kCanonPenaltyMiddle = 4;                         // NON_CANONICAL_PENALTY_MIDDLE (stage2.c:61)
constexpr int kCanonShifts = kCanonGreedyAdvance + kCanonMissBehind + 1;

#ifdef __HIPCC__
// 24 nucleotides from universal position start (>= -2): their 2-bit codes (nt j in bits 2j) and N flags
__device__ __forceinline__ void canon_window(const uint32_t* __restrict__ blocks, uint64_t nwords, int64_t start,
                                             uint64_t& codes, uint32_t& flags) {
  const unsigned under = start < 0 ? (unsigned)(-start) : 0u;  // positions in front of the genome
  const uint64_t s = start < 0 ? 0u : (uint64_t)start;
  const uint64_t ptr = s / 32u * 3u;
  const unsigned shift = (unsigned)(s % 32u);
  const uint64_t w0 = (uint64_t)me_word(blocks, nwords, ptr + 1) | ((uint64_t)me_word(blocks, nwords, ptr) << 32);
  const uint64_t w1 =
      (uint64_t)me_word(blocks, nwords, ptr + 4) | ((uint64_t)me_word(blocks, nwords, ptr + 3) << 32);
  const uint32_t f0 = me_word(blocks, nwords, ptr + 2), f1 = me_word(blocks, nwords, ptr + 5);
  uint64_t W = shift ? (w0 >> (2u * shift)) | (w1 << (64u - 2u * shift)) : w0;
  uint32_t F = shift ? (f0 >> shift) | (f1 << (32u - shift)) : f0;
  if (under) {
    W <<= 2u * under;
    F = (F << under) | ((1u << under) - 1u);
  }
  codes = W;
  flags = F;
}

// prevpos / currpos: the universal coordinates stage2.c:1258-1259 / 1286-1287 compute
// (evals: when given, counts the shifts whose two models were evaluated)
__device__ __forceinline__ bool canonical_link(const uint32_t* __restrict__ blocks, uint64_t nwords,
                                               const double* __restrict__ T, uint64_t prevpos, uint64_t currpos,
                                               bool plusp, uint64_t chroffset, unsigned* evals = nullptr) {
  const uint64_t floor = plusp ? (uint64_t)kCanonGreedyAdvance : (uint64_t)kCanonMissBehind;
  if (prevpos < floor || currpos < floor) return false;
  const uint64_t up = plusp ? (uint64_t)kCanonMissBehind : (uint64_t)kCanonGreedyAdvance;
  const uint64_t rL = (plusp ? prevpos : currpos) + up, rH = (plusp ? currpos : prevpos) + up;
  uint64_t cL, cH;
  uint32_t fL, fH;
  canon_window(blocks, nwords, (int64_t)rL - (kCanonShifts - 1), cL, fL);
  canon_window(blocks, nwords, (int64_t)rH - (kCanonShifts + 1), cH, fH);
  // dinucleotide codes (first nt in bits 0-1, second in bits 2-3; A 0, C 1, G 2, T 3)
  constexpr unsigned kGT = 2u | (3u << 2), kCT = 1u | (3u << 2), kAG = 0u | (2u << 2), kAC = 0u | (1u << 2);
  unsigned sense = 0, anti = 0;  // bit i: both dinucleotides at window index i (shift 22 - i)
  for (int i = 0; i < kCanonShifts; i++) {
    if (((fL >> i) & 3u) | ((fH >> i) & 3u)) continue;
    const unsigned dl = (unsigned)(cL >> (2 * i)) & 0xFu, dh = (unsigned)(cH >> (2 * i)) & 0xFu;
    if (dl == kGT && dh == kAG) sense |= 1u << i;
    if (dl == kCT && dh == kAC) anti |= 1u << i;
  }
  // the reference answers on the sense strand first; the order cannot change a boolean OR
  while (sense) {
    const int i = 31 - __clz((int)sense);  // descending positions, as the reference walks
    sense &= ~(1u << i);
    const uint64_t k = (uint64_t)(kCanonShifts - 1 - i);
    if (evals) ++*evals;
    if (maxent_prob(blocks, nwords, T, 0, rL - k, chroffset) > 0.9 &&
        maxent_prob(blocks, nwords, T, 1, rH - k, chroffset) > 0.9)
      return true;
  }
  while (anti) {
    const int i = 31 - __clz((int)anti);
    anti &= ~(1u << i);
    const uint64_t k = (uint64_t)(kCanonShifts - 1 - i);
    if (evals) ++*evals;
    if (maxent_prob(blocks, nwords, T, 2, rH - k, chroffset) > 0.9 &&
        maxent_prob(blocks, nwords, T, 3, rL - k, chroffset) > 0.9)
      return true;
  }
  return false;
}

// the link between the hit at chromosomal position prevposition (query distance qd before) and the hit at
// position, as range 2 sees it (indexsize_nt 8): stage2.c:1258-1259 (plus) / 1286-1287 (minus)
__device__ __forceinline__ bool canonical_hit_link(const uint32_t* __restrict__ blocks, uint64_t nwords,
                                                   const double* __restrict__ T, uint32_t prevposition,
                                                   uint32_t position, int qd, bool plusp, uint64_t chroffset,
                                                   uint64_t chrhigh, unsigned* evals = nullptr) {
  uint64_t prevpos, currpos;
  if (plusp) {
    prevpos = chroffset + prevposition + 8u;
    currpos = chroffset + position - (uint64_t)qd + 8u;
  } else {
    prevpos = chrhigh + 1u - prevposition - 8u;
    currpos = chrhigh + 1u - position + (uint64_t)qd - 8u;
  }
  return canonical_link(blocks, nwords, T, prevpos, currpos, plusp, chroffset, evals);
}
#endif

}  // namespace gmapdp
