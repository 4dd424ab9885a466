// pgpu_index_find -- where does this string occur, byte for byte, inside this stretch of the genomic sequence:
// the question the reference asks with strstr() over an intron (search_small_exon,
// src/factorization-refinement.c:781-834), answered for a batch of (pattern, window) queries from the index that is
// resident in HBM anyway.  Semantics: include/pintron_gpu.h; the wave-level routines: pgpu_find.h.
//
//   find_count   one wave per query: suffix-array interval of the pattern (k-mer table + lane-parallel bisection),
//                then the number of its entries inside the window -- or, when the window is smaller than the
//                interval (a short pattern in a short intron), the number of matches among the window's positions
//   (scan)       counts -> out_first (pgpu_exclusive_scan_u32, the scan of the pairing stage)
//   find_fill    one wave per query: the positions, ascending.  Window smaller than the interval, or more hits than
//                the LDS holds: lanes stride over the window, ballot + prefix popcount write the hits in order.
//                Otherwise the interval's entries inside the window are gathered in LDS, sorted there (bitonic, one
//                wave) and copied out.  Either way the work is bounded by the smaller of interval and window,
//                unless the answer itself is larger than the LDS.
#include "pgpu_find.h"
#include "pgpu_query_call.h"

namespace {

constexpr uint32_t FIND_SORT_CAP = 4096;          // positions one wave sorts in LDS (16 KB: ten workgroups per CU)

// window of a query as the kernels use it: occurrences t with first <= t <= last; empty when !valid
struct FindWindow { uint32_t first, last, len; bool valid; };
__device__ __forceinline__ FindWindow find_window(const pgpu_find_query& q, uint32_t n) {
  FindWindow w;
  const uint32_t hi = q.hi < n ? q.hi : n;            // hi is clamped to the sequence
  w.len = q.pat_len; w.first = q.lo;
  w.valid = q.pat_len > 0 && q.lo <= hi && q.pat_len <= hi - q.lo;
  w.last = w.valid ? hi - q.pat_len : 0;
  return w;
}

__global__ __launch_bounds__(64)
void find_count_kernel(const LcfIndexView ix, const uint8_t* __restrict__ pats, const pgpu_find_query* __restrict__ queries,
                       uint32_t* __restrict__ iv, uint32_t* __restrict__ cnt_out) {
  const uint32_t lane = threadIdx.x;
  const pgpu_find_query q = queries[blockIdx.x];
  const FindWindow w = find_window(q, ix.n);
  uint32_t a = 0, b = 0, cnt = 0;
  if (w.valid) {
    const uint8_t* __restrict__ P = pats + q.pat_off;
    find_sa_interval(ix, P, w.len, lane, &a, &b);
    const uint32_t width = w.last - w.first + 1;
    if (a < b && width < b - a) {                     // fewer window positions than occurrences in the sequence
      for (uint32_t base = 0; base < width; base += 64) {
        const uint32_t i = base + lane;
        const bool hit = i < width && find_match_at(ix.T, w.first + i, P, w.len);
        cnt += (uint32_t)__popcll(__ballot(hit));
      }
    } else {
      for (uint32_t k0 = a; k0 < b; k0 += 64) {
        const uint32_t k = k0 + lane;
        bool hit = false;
        if (k < b) { const uint32_t t = ix.sa[k]; hit = t >= w.first && t <= w.last; }
        cnt += (uint32_t)__popcll(__ballot(hit));
      }
    }
  }
  if (lane == 0) { iv[2 * blockIdx.x] = a; iv[2 * blockIdx.x + 1] = b; cnt_out[blockIdx.x] = cnt; }
}

__global__ __launch_bounds__(64)
void find_fill_kernel(const LcfIndexView ix, const uint8_t* __restrict__ pats, const pgpu_find_query* __restrict__ queries,
                      const uint32_t* __restrict__ iv, const unsigned long long* __restrict__ first, uint32_t* __restrict__ out) {
  __shared__ uint32_t buf[FIND_SORT_CAP];
  const uint32_t lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long o0 = first[blockIdx.x];
  const uint32_t cnt = (uint32_t)(first[blockIdx.x + 1] - o0);
  if (cnt == 0) return;
  const pgpu_find_query q = queries[blockIdx.x];
  const FindWindow w = find_window(q, ix.n);
  const uint8_t* __restrict__ P = pats + q.pat_off;
  const uint32_t a = iv[2 * blockIdx.x], b = iv[2 * blockIdx.x + 1];
  const uint32_t width = w.last - w.first + 1;
  uint32_t* __restrict__ dst = out + o0;
  if (width < b - a || cnt > FIND_SORT_CAP) {         // the window's positions in order: the hits come out ascending
    uint32_t done = 0;
    for (uint32_t base = 0; base < width; base += 64) {
      const uint32_t i = base + lane;
      const bool hit = i < width && find_match_at(ix.T, w.first + i, P, w.len);
      const unsigned long long m = __ballot(hit);
      const uint32_t slot = done + (uint32_t)__popcll(m & below);
      if (hit && slot < cnt) dst[slot] = w.first + i;
      done += (uint32_t)__popcll(m);
    }
    return;
  }
  uint32_t got = 0;                                    // the interval's entries inside the window, in suffix order
  for (uint32_t k0 = a; k0 < b; k0 += 64) {
    const uint32_t k = k0 + lane;
    uint32_t t = 0;
    bool hit = false;
    if (k < b) { t = ix.sa[k]; hit = t >= w.first && t <= w.last; }
    const unsigned long long m = __ballot(hit);
    const uint32_t slot = got + (uint32_t)__popcll(m & below);
    if (hit && slot < FIND_SORT_CAP) buf[slot] = t;
    got += (uint32_t)__popcll(m);
  }
  uint32_t p2 = 1;
  while (p2 < cnt) p2 <<= 1;                           // <= FIND_SORT_CAP, a power of two
  for (uint32_t i = cnt + lane; i < p2; i += 64) buf[i] = 0xFFFFFFFFu;
  __syncthreads();                                     // one wave per workgroup: orders the LDS traffic of its lanes
  for (uint32_t k = 2; k <= p2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = lane; i < p2; i += 64) {
        const uint32_t partner = i ^ j;
        if (partner > i) {
          const uint32_t x = buf[i], y = buf[partner];
          if ((x > y) == ((i & k) == 0)) { buf[i] = y; buf[partner] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = lane; i < cnt; i += 64) dst[i] = buf[i];
}

thread_local double t_find_ms[2] = {0.0, 0.0};

}  // namespace

extern "C" double pgpu_index_find_kernel_ms(int k) { return (k == 0 || k == 1) ? t_find_ms[k] : 0.0; }

extern "C" int pgpu_index_find(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns, size_t patterns_len,
                               const pgpu_find_query* queries, size_t n_queries,
                               uint32_t* out, size_t out_cap, uint64_t* out_first, size_t* n_out) {
  t_find_ms[0] = t_find_ms[1] = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  if (!ctx || !idx || !out_first || (n_queries && !queries) || (patterns_len && !patterns) || (!out && out_cap))
    return PGPU_EINVAL;
  if (n_queries > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 queries in one call");
  for (size_t i = 0; i < n_queries; ++i) {
    const pgpu_find_query& q = queries[i];
    if (q.reserved != 0 || q.lo > q.hi || q.pat_off > patterns_len || q.pat_len > patterns_len - q.pat_off)
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad find query (reserved != 0, lo > hi, or the pattern leaves the pattern buffer)");
  }
  if (n_out) *n_out = 0;
  out_first[0] = 0;
  if (n_queries == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;

  const LcfIndexView ix = pgpu_index_lcf_view(idx);
  const size_t nq = n_queries;
  // one allocation for everything whose size is known up front; the positions follow once they are counted
  const size_t o_q = up256(patterns_len + 64), o_iv = o_q + up256(nq * sizeof(pgpu_find_query)),
               o_cnt = o_iv + up256(2 * nq * sizeof(uint32_t)), o_first = o_cnt + up256((nq + 1) * sizeof(uint32_t)),
               o_tmp = o_first + up256((nq + 1) * sizeof(unsigned long long)), total_bytes = o_tmp + up256(pgpu_scan_tmp_bytes(nq + 1));
  const dim3 grid((unsigned)nq), blk(64);
  QueryCall call(ctx, "find");
  const hipStream_t st = call.st;
  TRY_HIP(hipMalloc((void**)&call.d, total_bytes));
  uint8_t* d_pats = call.d;
  pgpu_find_query* d_q = (pgpu_find_query*)(call.d + o_q);
  uint32_t* d_iv = (uint32_t*)(call.d + o_iv);
  uint32_t* d_cnt = (uint32_t*)(call.d + o_cnt);
  unsigned long long* d_first = (unsigned long long*)(call.d + o_first);
  void* d_tmp = call.d + o_tmp;
  TRY_HIP(call.timing_events(2));
  if (patterns_len) TRY_HIP(hipMemcpyAsync(d_pats, patterns, patterns_len, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(d_q, queries, nq * sizeof(pgpu_find_query), hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemsetAsync(d_cnt + nq, 0, sizeof(uint32_t), st));
  TRY_HIP(call.record(0));
  hipLaunchKernelGGL(find_count_kernel, grid, blk, 0, st, ix, d_pats, d_q, d_iv, d_cnt);
  pgpu_exclusive_scan_u32(d_cnt, d_first, nq + 1, d_tmp, st);
  TRY_HIP(call.record(1));
  TRY_HIP(hipMemcpyAsync(out_first, d_first, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  const unsigned long long total = out_first[nq];
  if (n_out) *n_out = (size_t)total;
  call.elapsed_ms(0, &t_find_ms[0]);
  // no failure of the stream: it has been waited for, and the caller repeats the call with room for *n_out
  if (total > out_cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "position buffer too small");
  if (total == 0) return PGPU_OK;
  TRY_HIP(hipMalloc((void**)&call.d2, (size_t)total * sizeof(uint32_t)));
  TRY_HIP(call.record(2));
  hipLaunchKernelGGL(find_fill_kernel, grid, blk, 0, st, ix, d_pats, d_q, d_iv, d_first, (uint32_t*)call.d2);
  TRY_HIP(call.record(3));
  TRY_HIP(hipMemcpyAsync(out, call.d2, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(1, &t_find_ms[1]);
  return PGPU_OK;
}
