// pc_expand.h -- host side of the compact pair stream (format: pc_kernel.hip's header comment): one list's
// ops back to its records.  Host-only C++ (no HIP include, no threads), so that a stand-alone program can
// include it; gmapdp_engine.cpp's expand_stream calls it once per list.
#ifndef GMAPDP_PC_EXPAND_H
#define GMAPDP_PC_EXPAND_H

#include <cstdint>
#include <cstring>

#include "../../include/gmapdp.h"

namespace gmapdp {

// The ops in [p, end) back to exactly m records at o (Rec: gmapdp_pair, 17-B RAW ops, or gmapdp_path_pair,
// 21-B RAW ops).  Reads nothing outside [p, end) and writes nothing outside o[0, m).  False when the ops do
// not decode to exactly m records and end - p bytes (o[0, m) may then be partly written).
template <typename Rec>
inline bool pc_expand_list(const uint8_t* p, const uint8_t* end, Rec* o, int m) {
  static const char nt[4] = {'A', 'C', 'G', 'T'}, cp[4] = {'*', '|', ' ', ':'};
  constexpr int kRaw = 1 + (int)sizeof(Rec);
  int k = 0;
  while (k < m && p < end) {
    if (*p == 0x02) {
      if (end - p < kRaw) return false;
      std::memcpy(&o[k++], p + 1, sizeof(Rec));
      p += kRaw;
      continue;
    }
    if (*p != 0x01 || end - p < 13) return false;
    int32_t q, g;
    std::memcpy(&q, p + 1, 4);
    std::memcpy(&g, p + 5, 4);
    const int dq = (int8_t)p[9], dg = (int8_t)p[10];
    const int len = p[11] | (p[12] << 8);
    p += 13;
    if (len == 0 || len > m - k) return false;
    for (int r = 0; r < len; r++, k++) {
      if (p >= end) return false;
      Rec& x = o[k];
      // (unsigned: a corrupted header must not overflow a signed int; valid streams never wrap)
      x.querypos = (int32_t)((uint32_t)q + (uint32_t)r * (uint32_t)dq);
      x.genomepos = (int32_t)((uint32_t)g + (uint32_t)r * (uint32_t)dg);
      if constexpr (sizeof(Rec) == sizeof(gmapdp_pair)) {
        x.jump = 0;
      } else {
        x.queryjump = 0;
        x.genomejump = 0;
      }
      if (*p == 0xFF) {
        if (end - p < 5) return false;
        std::memcpy(&x.cdna, p + 1, 4);
        p += 5;
      } else {
        const uint8_t b = *p++;
        if (b & 0xC0) return false;  // codes are 6 bits
        x.cdna = nt[b & 3];
        x.genome = x.genomealt = nt[(b >> 2) & 3];
        x.comp = cp[(b >> 4) & 3];
      }
    }
  }
  return k == m && p == end;
}

}  // namespace gmapdp

#endif
