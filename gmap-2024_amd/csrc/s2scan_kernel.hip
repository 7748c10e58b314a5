// s2scan_kernel.hip -- CDNA4 (gfx950) kernels for Stage2_scan (stage2.c:5610): the
// coverage count GMAP takes of every gregion before any Stage2_compute (stage3_from_gregions,
// gmap.c:1855-1899).
//
// Reference semantics restated (paths under the reference tree's src/):
//   Stage2_scan             stage2.c:5610 (one source: the major 8-mer oligoindex, diag_lookback 120,
//                           suffnconsecutive 20; coveredp all false; *stage2_source 1)
//   Oligoindex_hr_tally + Oligoindex_get_mappings   as oi_kernel.hip restates them
//   Diag_update_coverage    diag.c:216 (scores[querystart] += 1, scores[queryend] -= 1 per diagonal; a
//                           position is covered where the running sum is > 0; ncovered counts them)
//
// Design.  Three launches per sub-batch, one block per (read, window):
//   s2scan_gather_kernel  copies each problem's query slice into the sub-batch's private query arena, so
//                         that the per-position arrays the seeding keys by query offset (npositions,
//                         mappings) are per problem even when several problems share one slice of the
//                         caller's arena (a read's gregions all do); it also resets the event pool's cursor;
//   s2scan_table_kernel   oi_kernel's pass (oi_pass, unchanged) under a name of its own: the table, the
//                         per-position values, cum_nohits;
//   s2scan_kernel         one wave: oi_mappings_global as oi_map_kernel runs it (same LDS: the radix
//                         histogram, the event step's offsets, the slot filter), the good-diagonal records
//                         into the problem's scratch, then the coverage count in the same wave and the 16-byte
//                         result.  The coverage bitmap (one bit per query position) aliases the radix
//                         histogram, which is free once the diagonals are out: no LDS is added to
//                         oi_map_kernel's 9 KB, so as many waves share a CU.  Queries past kScanBitmapBits
//                         positions take a difference array in the problem's cum_nohits slice (free by then
//                         as well), as s2c_kernel does.
// Nothing but the gmapdp_scan_result leaves the device.
#undef GMAPDP_OI_TIMING  // (the phase marks are the seeding kernels' own)
#define GMAPDP_OI_DEVICE_ONLY
#include "oi_kernel.hip"

namespace gmapdp {

// per problem, beside its DevOligoProblem (whose qoff is the private arena's): the caller's query slice and
// the result slot in the caller's order (DevOligoProblem.index is the slot within the sub-batch)
struct DevScanExtra {
  int32_t src_qoff;
  int32_t out_index;
};

constexpr int kScanGatherThreads = 256;
__global__ __launch_bounds__(kScanGatherThreads) void s2scan_gather_kernel(
    const DevOligoProblem* __restrict__ probs, const DevScanExtra* __restrict__ extra,
    const char* __restrict__ quc_all, char* __restrict__ quc_priv, unsigned long long* __restrict__ pool_counter) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *pool_counter = 0ull;
  const int qlen = probs[blockIdx.x].querylength;
  const char* src = quc_all + extra[blockIdx.x].src_qoff;
  char* dst = quc_priv + probs[blockIdx.x].qoff;
  for (int i = threadIdx.x; i < qlen; i += kScanGatherThreads) dst[i] = src[i];
}

template <typename CT, bool kModal>
__global__ __launch_bounds__(64 * kOiWaves) void s2scan_table_kernel(OI_PASS_ARGS) {
  oi_pass<CT, kModal>(probs, blocks, quc_all, scratch, results, npos_out, map_out, table_all, pool_counter, pool_cap,
                      nhits_out);
}

template <bool kModal>  // the long class (oi_long_kernel's pass)
__global__ __launch_bounds__(64 * kOiWaves) void s2scan_table_long_kernel(OI_PASS_ARGS) {
  oi_pass<uint32_t, kModal, true>(probs, blocks, quc_all, scratch, results, npos_out, map_out, table_all, pool_counter,
                                  pool_cap, nhits_out);
}

// query positions the LDS bitmap holds (512 B of the 4-KB histogram); longer queries: the global difference array
constexpr int kScanBitmapBits = 4096;
static_assert(kScanBitmapBits / 32 <= kOiHist, "the coverage bitmap aliases the radix histogram");

__global__ __launch_bounds__(64) void s2scan_kernel(
    const DevOligoProblem* __restrict__ probs, const DevScanExtra* __restrict__ extra,
    unsigned char* __restrict__ scratch, gmapdp_oligo_result* __restrict__ ores,
    const int32_t* __restrict__ npos_all, const int32_t* __restrict__ map_all, const uint32_t* __restrict__ table_all,
    int32_t* __restrict__ diag_all, uint64_t* __restrict__ pool, gmapdp_scan_result* __restrict__ out,
    int32_t* __restrict__ overflow_flag) {
  __shared__ uint32_t hist[kOiHist];
  __shared__ int evq[3 * 256];
  __shared__ uint32_t slots[kOimSlots / 2];
  const int lane = threadIdx.x;
  const DevOligoProblem P = probs[blockIdx.x];
  const int qlen = P.querylength;
  const int nq = qlen - kOiK + 1;
  unsigned char* base_s = scratch + P.scratch_offset;
  const gmapdp_oligo_result tally = ores[P.index];  // s2scan_table_kernel's record
  int32_t* good = diag_all + 4 * P.diag_offset;
  int ndiag = 0, maxn = 0;
  bool overflow = tally.oned_matrix_p < 0;
  if (!overflow && P.chrend > P.chrstart) {  // (else get_mappings returns before writing anything)
    const ScratchOi so = scratch_oi(qlen, P.chrend - P.chrstart);
    oi_mappings_global<true>(lane, P, scratch, qlen, nq, tally.totalpositions, npos_all + P.qoff, map_all + P.qoff,
                             reinterpret_cast<const int*>(base_s), table_all + P.table_offset, pool,
                             *reinterpret_cast<const unsigned long long*>(base_s + so.poolbase), hist, evq, good, ores,
                             slots);
    // lane 0 wrote the record; the lanes' diagonal records are read by other lanes below
    int nd0 = 0, mx0 = 0, on0 = 0;
    if (lane == 0) {
      nd0 = ores[P.index].ndiagonals;
      mx0 = ores[P.index].maxnconsecutive;
      on0 = ores[P.index].oned_matrix_p;
    }
    ndiag = __builtin_amdgcn_readfirstlane(nd0);
    maxn = __builtin_amdgcn_readfirstlane(mx0);
    overflow = __builtin_amdgcn_readfirstlane(on0) < 0;
    __threadfence_block();
    oi_wave_sync();
  }
  // (a problem's layout gives it diag_cap records; get_mappings reports more than that as overflow)
  ndiag = min(ndiag, (int)min(P.diag_cap, 0x7fffffffu));

  // ---- Diag_update_coverage with coveredp all false ----
  int ncovered = 0;
  if (!overflow && ndiag > 0) {
    if (qlen <= kScanBitmapBits) {
      // the union of the [querystart, queryend) ranges as a bitmap: lanes take diagonals, 64 at a time
      uint32_t* bm = hist;
      const int nw = (qlen + 31) >> 5;
      for (int w = lane; w < nw; w += 64) bm[w] = 0u;
      oi_wave_sync();
      for (int d = lane; d < ndiag; d += 64) {
        const int4 r = reinterpret_cast<const int4*>(good)[d];
        const int qs = max(r.y, 0), qe = min(r.z, qlen);  // clipped: never a bit outside the query
        if (qs < qe) {
          const int w0 = qs >> 5, w1 = (qe - 1) >> 5;
          const uint32_t first = 0xFFFFFFFFu << (qs & 31), last = 0xFFFFFFFFu >> (31 - ((qe - 1) & 31));
          if (w0 == w1) {
            atomicOr(&bm[w0], first & last);
          } else {
            atomicOr(&bm[w0], first);
            for (int w = w0 + 1; w < w1; w++) atomicOr(&bm[w], 0xFFFFFFFFu);
            atomicOr(&bm[w1], last);
          }
        }
      }
      oi_wave_sync();
      int c = 0;
      for (int w = lane; w < nw; w += 64) c += __popc(bm[w]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
      ncovered = c;
    } else {
      // the reference's difference array over [0, querylength], in the problem's cum_nohits slice
      int* diff = reinterpret_cast<int*>(base_s);
      for (int q = lane; q <= qlen; q += 64) diff[q] = 0;
      __threadfence_block();
      oi_wave_sync();
      for (int d = lane; d < ndiag; d += 64) {
        const int4 r = reinterpret_cast<const int4*>(good)[d];
        atomicAdd(&diff[min(max(r.y, 0), qlen)], 1);
        atomicAdd(&diff[min(max(r.z, 0), qlen)], -1);
      }
      __threadfence_block();
      oi_wave_sync();
      int carry = 0, c = 0;
      for (int cb = 0; cb < qlen; cb += 64) {
        const int q = cb + lane;
        int depth = q < qlen ? diff[q] : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int y = __shfl_up(depth, off, 64);
          if (lane >= off) depth += y;
        }
        depth += carry;
        carry = __shfl(depth, 63, 64);
        c += (q < qlen && depth > 0) ? 1 : 0;
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
      ncovered = c;
    }
  }
  if (lane == 0) {
    gmapdp_scan_result R;
    // a seeding layout overflow is never a count: ncovered -1, stage2_source 0, and the batch's flag
    R.ncovered = overflow ? -1 : ncovered;
    R.stage2_source = overflow ? 0 : 1;
    R.totalpositions = tally.totalpositions;
    R.maxnconsecutive = overflow ? 0 : maxn;
    out[extra[blockIdx.x].out_index] = R;
    if (overflow) *overflow_flag = 1;
  }
}

// One sub-batch: gather, table, scan, in stream order.  `extra` as raw bytes (DevScanExtra is this file's).
hipError_t launch_s2scan(bool wide, bool modal, bool longq, int nproblems, size_t lds, hipStream_t stream,
                         const DevOligoProblem* probs, const void* extra, const uint32_t* blocks, const char* quc_all,
                         char* quc_priv, unsigned char* scratch, gmapdp_oligo_result* ores, int32_t* npos, int32_t* map,
                         uint32_t* table, int32_t* diags, uint64_t* pool, unsigned long long* pool_counter,
                         unsigned long long pool_cap, gmapdp_scan_result* out, int32_t* overflow_flag) {
  const DevScanExtra* ex = static_cast<const DevScanExtra*>(extra);
  hipLaunchKernelGGL(s2scan_gather_kernel, dim3(nproblems), dim3(kScanGatherThreads), 0, stream, probs, ex, quc_all,
                     quc_priv, pool_counter);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  void* fn = longq ? (modal ? reinterpret_cast<void*>(&s2scan_table_long_kernel<true>)
                            : reinterpret_cast<void*>(&s2scan_table_long_kernel<false>))
             : modal ? (wide ? reinterpret_cast<void*>(&s2scan_table_kernel<uint32_t, true>)
                           : reinterpret_cast<void*>(&s2scan_table_kernel<uint16_t, true>))
                   : (wide ? reinterpret_cast<void*>(&s2scan_table_kernel<uint32_t, false>)
                           : reinterpret_cast<void*>(&s2scan_table_kernel<uint16_t, false>));
  if (lds > 64 * 1024) {
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const char* quc = quc_priv;
  int32_t* nhits_out = nullptr;
  void* args[] = {(void*)&probs, (void*)&blocks, (void*)&quc, (void*)&scratch, (void*)&ores, (void*)&npos,
                  (void*)&map, (void*)&table, (void*)&pool_counter, (void*)&pool_cap, (void*)&nhits_out};
  e = hipLaunchKernel(fn, dim3(nproblems), dim3(64 * kOiWaves), args, lds, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(s2scan_kernel, dim3(nproblems), dim3(64), 0, stream, probs, ex, scratch, ores,
                     (const int32_t*)npos, (const int32_t*)map, (const uint32_t*)table, diags, pool, out, overflow_flag);
  return hipGetLastError();
}

}  // namespace gmapdp
