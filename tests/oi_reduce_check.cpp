// oi_reduce_check.cpp -- host check of csrc/oi_reduce.h (tests/test_stage2_modes_power.py builds it with
// -fsanitize=address,undefined and runs it): every bit formula against a per-nucleotide loop over the sixteen
// 2-bit codes of a word, for all 2^16 patterns in either half (the other half zero, all ones, and the same
// pattern), the masked 64-bit form the kernels use, and the (mode, plusp) -> reduction table.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../gmap-2024_amd/csrc/oi_reduce.h"

using namespace gmapdp;

// A=0 C=1 G=2 T=3, one code at a time (cmet.c / atoi.c: convert_ct, _ga, _tc, _ag act per nucleotide)
static uint32_t by_nucleotide(uint32_t x, int red) {
  uint32_t out = 0;
  for (int i = 0; i < 16; i++) {
    uint32_t c = (x >> (2 * i)) & 3u;
    if (red == kRedCT && c == 1) c = 3;
    if (red == kRedGA && c == 2) c = 0;
    if (red == kRedTC && c == 3) c = 1;
    if (red == kRedAG && c == 0) c = 2;
    out |= c << (2 * i);
  }
  return out;
}

int main() {
  long checked = 0, bad = 0;
  uint32_t (*const formula[5])(uint32_t) = {nullptr, oi_reduce_ct, oi_reduce_ga, oi_reduce_tc, oi_reduce_ag};
  for (int red = kRedNone; red <= kRedAG; red++) {
    const OiReduceMasks m = oi_reduce_masks(red);
    for (uint32_t p = 0; p < 65536u; p++) {
      const uint32_t words[6] = {p, p << 16, p | 0xFFFF0000u, (p << 16) | 0xFFFFu, p | (p << 16), ~p};
      for (uint32_t x : words) {
        const uint32_t want = by_nucleotide(x, red);
        const uint32_t got = red ? formula[red](x) : x;
        const uint64_t v = (uint64_t)x | ((uint64_t)~x << 32);  // two different half-words of one funnel
        const uint64_t want64 = (uint64_t)want | ((uint64_t)by_nucleotide(~x, red) << 32);
        if (got != want || oi_reduce(x, red) != want || oi_reduce64(v, m) != want64) {
          if (bad++ < 8) std::printf("reduction %d of %08x: %08x, per nucleotide %08x\n", red, x, got, want);
        }
        checked++;
      }
    }
  }
  // Mode_T 0..6; the stranded modes' rows as count / store_positions_fwd_std (plus) and _rev_std (minus)
  // apply them (oligoindex_hr.c:19293-19320, :30795-30821); the non-stranded modes have no reduction here
  const int table[7][2] = {{kRedNone, kRedNone}, {kRedCT, kRedGA}, {-1, -1}, {kRedTC, kRedAG},
                           {-1, -1},             {kRedAG, kRedTC}, {-1, -1}};
  for (int mode = -1; mode <= 7; mode++)
    for (int plusp = 0; plusp < 2; plusp++) {
      const int want = (mode < 0 || mode > 6) ? -1 : table[mode][plusp ? 0 : 1];
      if (oi_reduction_of(mode, plusp != 0) != want) {
        std::printf("mode %d plusp %d: reduction %d, expected %d\n", mode, plusp, oi_reduction_of(mode, plusp != 0), want);
        bad++;
      }
      checked++;
    }
  // in read orientation (the minus strand's words complemented: code c -> 3 - c) both strands reduce alike
  for (int mode : {1, 3, 5})
    for (uint32_t c = 0; c < 4; c++) {
      const uint32_t plus = oi_reduce(c, oi_reduction_of(mode, true)) & 3u;
      const uint32_t minus = 3u - (oi_reduce(3u - c, oi_reduction_of(mode, false)) & 3u);
      if (plus != minus) {
        std::printf("mode %d code %u: plus %u, minus (read orientation) %u\n", mode, c, plus, minus);
        bad++;
      }
      checked++;
    }
  std::printf("%ld checks, %ld bad\n", checked, bad);
  return bad ? 1 : 0;
}
