// pc_expand_check.cpp -- the host decoder of the compact pair stream (csrc/pc_expand.h) under a memory
// checker: a stand-alone program, built by tests/test_pair_stream.py with -fsanitize=address,undefined.
// It reads a case file (written by the test with the Python reference encoder): "PCX1", uint32 cases, then
// per case uint8 is_path_pairs, uint32 records, uint32 stream bytes, the records, the stream.  For every case
// the whole stream, every proper prefix of it and single-byte corruptions go, each in a heap buffer of
// exactly its size, through pc_expand_list into an arena of exactly the list's records.  The whole stream
// must give the exact records and a prefix must be refused.  A corrupted byte may leave a valid stream of
// other records (a code, a position or an escaped character has no redundancy), so there the decoder must
// give the exact records or accept exactly when the ops are still well formed (well_formed below walks the
// ops without decoding them).  Exit status 0 and no sanitizer report: pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gmap-2024_amd/csrc/pc_expand.h"
#include "../include/gmapdp.h"

static long g_calls = 0, g_refused = 0, g_other = 0;

// one decode of `n` stream bytes into `m` records, both buffers exactly sized; 1: exact records, 0: refused
template <typename Rec>
static int decode_once(const uint8_t* src, size_t n, const uint8_t* want, int m, int m_expected) {
  uint8_t* s = (uint8_t*)std::malloc(n ? n : 1);
  if (n) std::memcpy(s, src, n);
  Rec* out = (Rec*)std::malloc(m ? sizeof(Rec) * (size_t)m : 1);
  if (m) std::memset(out, 0x5A, sizeof(Rec) * (size_t)m);
  // (an empty stream: a pointer one past a live byte, never dereferenced)
  const uint8_t* p = n ? s : s + 1;
  const bool ok = gmapdp::pc_expand_list<Rec>(p, p + n, out, m);
  g_calls++;
  int r = 0;
  if (ok) {
    if (m != m_expected || (m && std::memcmp(out, want, sizeof(Rec) * (size_t)m) != 0)) {
      g_other++;
      r = -1;
    } else {
      r = 1;
    }
  } else {
    g_refused++;
  }
  std::free(out);
  std::free(s);
  return r;
}

// whether n bytes are ops for exactly m records: the format's structure alone
static bool well_formed(const uint8_t* s, size_t n, long m, size_t recsize) {
  size_t p = 0;
  long k = 0;
  while (k < m && p < n) {
    if (s[p] == 0x02) {
      if (n - p < 1 + recsize) return false;
      p += 1 + recsize;
      k++;
    } else if (s[p] == 0x01) {
      if (n - p < 13) return false;
      const long len = s[p + 11] | (s[p + 12] << 8);
      p += 13;
      if (len == 0 || len > m - k) return false;
      for (long r = 0; r < len; r++) {
        if (p >= n) return false;
        if (s[p] == 0xFF) {
          if (n - p < 5) return false;
          p += 5;
        } else if (s[p] & 0xC0) {
          return false;
        } else {
          p++;
        }
      }
      k += len;
    } else {
      return false;
    }
  }
  return k == m && p == n;
}

template <typename Rec>
static int check_case(int ci, const uint8_t* recs, int m, const uint8_t* stream, size_t n) {
  int bad = 0;
  if (decode_once<Rec>(stream, n, recs, m, m) != 1) {
    std::fprintf(stderr, "case %d: the whole stream does not decode to its records\n", ci);
    bad++;
  }
  // a list of another length must be refused
  if (decode_once<Rec>(stream, n, recs, m + 1, m) != 0) bad++;
  if (m > 0 && decode_once<Rec>(stream, n, recs, m - 1, m) != 0) bad++;
  for (size_t k = 0; k < n; k++) {  // every proper prefix
    if (decode_once<Rec>(stream, k, recs, m, m) != 0) {
      std::fprintf(stderr, "case %d: the prefix of %zu bytes is not refused\n", ci, k);
      bad++;
    }
  }
  // single-byte corruptions: every position of a short stream, else the first 48 and a stride
  std::vector<uint8_t> c(stream, stream + n);
  const size_t stride = n > 144 ? n / 96 : 1;
  for (size_t k = 0; k < n; k++) {
    if (k >= 48 && k % stride) continue;
    const uint8_t o = c[k];
    const uint8_t vals[] = {0x00, 0x01, 0x02, 0x03, 0x3F, 0x40, 0x7F, 0x80, 0xFE, 0xFF, (uint8_t)(o + 1),
                            (uint8_t)(o - 1), (uint8_t)(o ^ 0x80)};
    for (uint8_t v : vals) {
      if (v == o) continue;
      c[k] = v;
      const int r = decode_once<Rec>(c.data(), n, recs, m, m);
      if (r != 1 && (r != 0) != well_formed(c.data(), n, m, sizeof(Rec))) {
        std::fprintf(stderr, "case %d: byte %zu set to 0x%02x: %s\n", ci, k, v,
                     r ? "accepted, though the ops are malformed" : "refused, though the ops are well formed");
        bad++;
      }
    }
    c[k] = o;
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  size_t got;
  while ((got = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  std::fclose(f);
  if (buf.size() < 8 || std::memcmp(buf.data(), "PCX1", 4) != 0) {
    std::fprintf(stderr, "not a case file\n");
    return 2;
  }
  uint32_t ncases;
  std::memcpy(&ncases, buf.data() + 4, 4);
  size_t at = 8;
  int bad = 0;
  for (uint32_t ci = 0; ci < ncases; ci++) {
    if (buf.size() - at < 9) return 2;
    const int path = buf[at];
    uint32_t m, n;
    std::memcpy(&m, buf.data() + at + 1, 4);
    std::memcpy(&n, buf.data() + at + 5, 4);
    at += 9;
    const size_t rb = (size_t)m * (path ? sizeof(gmapdp_path_pair) : sizeof(gmapdp_pair));
    if (buf.size() - at < rb + n) return 2;
    const uint8_t* recs = buf.data() + at;
    const uint8_t* stream = recs + rb;
    at += rb + n;
    bad += path ? check_case<gmapdp_path_pair>((int)ci, recs, (int)m, stream, n)
                : check_case<gmapdp_pair>((int)ci, recs, (int)m, stream, n);
  }
  if (at != buf.size()) return 2;
  std::printf("%u cases, %ld decodes, %ld refused, %ld to other records, %d wrong\n", ncases, g_calls, g_refused,
              g_other, bad);
  return bad ? 1 : 0;
}
