// oi_reduce.h -- the genome reductions of GMAP's cmet / atoi / ttoc modes (host and device).
//
// Oligoindex_hr_tally reduces every genome word before it extracts 8-mers (count_positions_fwd_std
// oligoindex_hr.c:19293-19320, _rev_std :30795-30821, and the store passes alike); the query is not
// reduced.  A word holds sixteen 2-bit codes (A=0 C=1 G=2 T=3) and each code is reduced on its own
// (cmet.c / atoi.c: Cmet_reduce_ct C->T, _ga G->A, Atoi_reduce_tc T->C, _ag A->G), so every reduction is
// a rewrite of the code's high bit from its low bit:
//   ct 01->11: high |= low      ag 00->10: high |= ~low
//   ga 10->00: high &= low      tc 11->01: high &= ~low
// The flags word is not consulted: an N's stored code is reduced like any other.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OI_REDUCE_HD __host__ __device__ inline
#else
#define OI_REDUCE_HD inline
#endif

namespace gmapdp {

enum OiReduction : int32_t { kRedNone = 0, kRedCT = 1, kRedGA = 2, kRedTC = 3, kRedAG = 4 };

OI_REDUCE_HD uint32_t oi_reduce_ct(uint32_t x) { return x | ((x & 0x55555555u) << 1); }
OI_REDUCE_HD uint32_t oi_reduce_ga(uint32_t x) { return x & (((x & 0x55555555u) << 1) | 0x55555555u); }
OI_REDUCE_HD uint32_t oi_reduce_tc(uint32_t x) { return x & ~((x & 0x55555555u) << 1); }
OI_REDUCE_HD uint32_t oi_reduce_ag(uint32_t x) { return x | ((~x & 0x55555555u) << 1); }

OI_REDUCE_HD uint32_t oi_reduce(uint32_t x, int red) {
  return red == kRedCT ? oi_reduce_ct(x) : red == kRedGA ? oi_reduce_ga(x) : red == kRedTC ? oi_reduce_tc(x)
         : red == kRedAG ? oi_reduce_ag(x) : x;
}

// Mode_T (mode.h): STANDARD 0, CMET_STRANDED 1, CMET_NONSTRANDED 2, ATOI_STRANDED 3, ATOI_NONSTRANDED 4,
// TTOC_STRANDED 5, TTOC_NONSTRANDED 6.  The stranded modes' reduction of the forward-strand words of a
// plus- / minus-strand window (in read orientation both strands reduce alike: C->T, T->C, A->G); the
// non-stranded modes have none here (-1: the engine refuses stage 2 in them).
OI_REDUCE_HD int oi_reduction_of(int mode, bool plusp) {
  switch (mode) {
    case 0: return kRedNone;
    case 1: return plusp ? kRedCT : kRedGA;
    case 3: return plusp ? kRedTC : kRedAG;
    case 5: return plusp ? kRedAG : kRedTC;
    default: return -1;
  }
}

// The same reductions with the selection in three wave-uniform masks, over the 64-bit pair of half-words the
// seeding kernels funnel their 8-mers from: l = the low bits moved onto the high bits, inverted for ag / tc;
// the or-type reductions (ct, ag) set the high bit from it, the and-type ones (ga, tc) clear it.
struct OiReduceMasks {
  uint64_t inv, orm, andm;
};
OI_REDUCE_HD OiReduceMasks oi_reduce_masks(int red) {
  constexpr uint64_t kHi = 0xAAAAAAAAAAAAAAAAull, kLo = 0x5555555555555555ull;
  OiReduceMasks m;
  m.inv = (red == kRedAG || red == kRedTC) ? kHi : 0ull;
  m.orm = (red == kRedCT || red == kRedAG) ? kHi : 0ull;
  m.andm = (red == kRedGA || red == kRedTC) ? kLo : ~0ull;
  return m;
}
OI_REDUCE_HD uint64_t oi_reduce64(uint64_t v, const OiReduceMasks& m) {
  const uint64_t l = ((v & 0x5555555555555555ull) << 1) ^ m.inv;
  return (v | (l & m.orm)) & (l | m.andm);
}

}  // namespace gmapdp
