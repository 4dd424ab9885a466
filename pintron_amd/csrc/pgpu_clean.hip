// A candidate factorization's cleaning steps, chained, on the resident index.  Semantics: include/pintron_gpu.h
// (pgpu_index_clean_chains): one query is one candidate of get_EST_factorizations (src/est-factorizations.c:212-244), and
// the answer is the verdict of the six steps with the list as they left it.
//
//   clean_kernel    one wave per query; a wave that has finished a query takes the next one of its stride.  The exons sit
//                   in the wave's LDS, one lane loads one; the list is always a run [lo, hi) of them (the steps only drop
//                   at the ends or keep one run), the flagged exons of steps 4 and 5 are a 64-bit ballot, and the best-run
//                   rule is a scan over its set bits.  Without the host in between:
//                     endpoints  lev_wave_body<1, ALIGN> + align_traceback_wave, or align_band_sweep + align_band_traceback,
//                                of pgpu_wave_dp.h on a DevJob built here -- the code and the choice of the PGPU_DP_ALIGN
//                                jobs of a plan -- then head_walk_window / tail_walk_window / close_tail_gaps over the two
//                                gapped rows, 64 columns at a time: the walks of endpoint_epilogue, here over every window;
//                     external   lengths, splice-site bytes and a byte comparison: no DP;
//                     dust       dust_flags_wave per exon;
//                     noisy      lev_wave_body<1, KBAND> per exon (kband_band_sweep, or the whole matrix of a short exon).
//                   Divergence is per query: everything that decides is uniform over the wave.
//                   The direction words and the two gapped rows live in a per-wave workspace in HBM inside the call's one
//                   allocation, sized by the host for the longest end exon of the call; the traceback's window is in LDS
//                   (DESIGN.md section 5g).
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_wave_dp.h"
#include "pgpu_clean_body.h"
#include "pgpu_stage_launch.h"

namespace {

constexpr uint32_t MAX_EXONS = PGPU_CLEAN_MAX_EXONS;
constexpr uint32_t MAX_END = PGPU_CLEAN_MAX_END_EXON;
constexpr uint32_t MAX_KBAND = 31;                     // 2k + 1 <= 64 diagonals on the lanes (kband_band_sweep)
static_assert(MAX_EXONS == 64, "one lane per exon, one ballot bit per exon");
static_assert(ALIGN_BAND_K == MAX_KBAND, "both bands take the whole wave");

// (dirs_wave, dirs_band, rows_bytes -- the direction bytes and the two rows of one end-exon alignment -- are in
// pgpu_stage_launch.h, with the rule that sizes the workspace from them)

struct CleanLds {
  __attribute__((aligned(16))) uint8_t win[TB_WIN_BYTES];   // the traceback's direction window ...
  uint8_t path[TB_PATH];                                    // ... and path
  pgpu_factor ex[MAX_EXONS];                                // the query's exons as the steps leave them
  uint8_t marks[MAX_EXONS];
};

// the two gapped rows in the wave's workspace (a 0 follows each row)
struct MemRows {
  uint8_t* ea; uint8_t* ga;
  __device__ __forceinline__ uint32_t e(uint32_t q) const { return ea[q]; }
  __device__ __forceinline__ uint32_t g(uint32_t q) const { return ga[q]; }
  __device__ __forceinline__ void set_e(uint32_t q, uint32_t v) { ea[q] = (uint8_t)v; }
  __device__ __forceinline__ void set_g(uint32_t q, uint32_t v) { ga[q] = (uint8_t)v; }
};

// (best_run, the best-run rule of steps 4 and 5, and external_exon_ok, the test of step 3: pgpu_clean_body.h)

__global__ __launch_bounds__(64)
void clean_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint8_t* __restrict__ ests, const pgpu_factor* __restrict__ exons,
                  const pgpu_clean_query* __restrict__ queries, uint32_t n_queries, uint8_t* __restrict__ ws,
                  const size_t ws_dirs, const size_t ws_rows, pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_marks,
                  pgpu_clean_result* __restrict__ out, uint32_t* __restrict__ undersized) {
  __shared__ CleanLds S;
  const uint32_t lane = threadIdx.x;
  const size_t ws_wave = (ws_dirs + ws_rows + sizeof(DevResult) + 255) & ~(size_t)255;
  uint8_t* const w = ws + (size_t)blockIdx.x * ws_wave;
  DevResult* const res = reinterpret_cast<DevResult*>(w + ws_dirs + ws_rows);
  for (uint32_t c = blockIdx.x; c < n_queries; c += gridDim.x) {
    const pgpu_clean_query q = queries[c];
    const uint8_t* const est = ests + q.est_off;
    const uint32_t ne = q.n_exons;
    pgpu_clean_result cr;
    cr.status = PGPU_OK; cr.verdict = 0; cr.first_kept = 0; cr.n_kept = 0;
    uint32_t lo = 0, hi = ne;
    bool refused = ne > MAX_EXONS;
    __syncthreads();                                           // the query before is done with the LDS
    if (!refused && lane < ne) { S.ex[lane] = exons[q.first_exon + lane]; S.marks[lane] = 0; }
    __syncthreads();
    // ---- step 1: check_for_not_source_sink_factorization (:2111-2125), check_exon_start_end (:1989-2019)
    if (!refused) {
      if (ne == 1 && (S.ex[0].EST_start < 0 || (uint32_t)S.ex[0].EST_start >= q.est_len)) cr.verdict = 1;
      else {
        bool bad = false;
        if (lane < ne) {
          const pgpu_factor f = S.ex[lane];
          const int pe = lane ? S.ex[lane - 1].EST_end : -1, pg = lane ? S.ex[lane - 1].GEN_end : -1;
          bad = f.EST_start > f.EST_end || f.GEN_start > f.GEN_end || f.EST_start < pe || f.GEN_start < pg;
        }
        if (__any(bad)) cr.verdict = 2;
      }
    }
    // ---- step 2: handle_endpoints (:2127-2301): end 0 the head, end 1 the tail (of the list as the head left it)
    for (uint32_t end = 0; end < 2 && !refused && cr.verdict == 0; ++end) {
      const uint32_t at = end == 0 ? lo : hi - 1;
      const pgpu_factor f = S.ex[at];
      const uint32_t la = (uint32_t)(f.EST_end - f.EST_start + 1), lb = (uint32_t)(f.GEN_end - f.GEN_start + 1);
      if (la > MAX_END || lb > MAX_END) { refused = true; break; }
      DevJob job;
      job.a = est + f.EST_start; job.b = T + f.GEN_start; job.la = la; job.lb = lb;
      job.p0 = job.p1 = job.p2 = job.tail = 0;
      job.ws_off = 0; job.str_off = ws_dirs; job.out_idx = 0; job.r_class = 1;
      // The host sized the workspace for every alignment a query of this call can reach (the loop in the entry), so none
      // of the three size tests below can fire today.  They keep a later slip in that sizing from writing out of bounds,
      // and it does not pass for a refusal: the call then fails as a whole with PGPU_EDEVICE.
      const bool band = la > 64u && (la > lb ? la - lb : lb - la) <= ALIGN_BAND_HALF;
      if (rows_bytes(la, lb) > ws_rows || (la <= 64u && dirs_wave(lb) > ws_dirs) || (band && dirs_band(la) > ws_dirs)) {
        if (lane == 0) atomicOr(undersized, 1u);
        refused = true; break;
      }
      if (la <= 64u) {                                                      // lev_wave<ALIGN>
        lev_wave_body<1, MODE_ALIGN>(job, res, w, lane);
        own_stores_visible();
        align_traceback_wave(job, res, w, w, lane, S.win, S.path);
      } else {                                                              // align_band, settled inside the band or refused
        if (!band) { refused = true; break; }
        bool same = la == lb;
        if (same) for (uint32_t k = lane; k < la; k += 64) same = same && job.a[k] == job.b[k];
        if (__all(same)) {                                                  // identity alignment (compute-alignments.c:48-58)
          if (lane == 0) { res->status = 0; res->v[0] = 0; res->v[1] = (int32_t)la; res->v[5] = 1; }
          own_stores_visible();
          align_traceback_wave(job, res, w, w, lane, S.win, S.path);        // its identity branch
        } else {
          uint32_t* const bdirs = reinterpret_cast<uint32_t*>(w);
          const uint32_t score = align_band_sweep(job.a, la, job.b, lb, lane, bdirs);
          if (score > ALIGN_BAND_K) { refused = true; break; }
          if (lane == 0) { res->status = 0; res->v[0] = (int32_t)score; res->v[5] = 0; }
          own_stores_visible();
          align_band_traceback(job, res, bdirs, w, lane, S.win, S.path);
        }
      }
      own_stores_visible();                                                 // the two rows and their length
      const uint32_t dim = (uint32_t)__builtin_amdgcn_readfirstlane(res->v[1]);
      uint8_t* const ea = w + (uint32_t)__builtin_amdgcn_readfirstlane((int)res->str[0]);
      uint8_t* const ga = w + (uint32_t)__builtin_amdgcn_readfirstlane((int)res->str[1]);
      __syncthreads();                                                      // the traceback is done with the window
      if (end == 0) {
        uint32_t matches = 0, cf = 0, ce = 0;
        bool stop = false;
        for (uint32_t base = 0; base < dim && !stop; base += 64) {
          const uint32_t col = base + lane;
          const uint32_t xe = col < dim ? ea[col] : 0u, xg = col < dim ? ga[col] : 0u;
          const unsigned long long eq = __ballot(col < dim && xe == xg), eg = __ballot(xe == '-'), gg = __ballot(xg == '-');
          head_walk_window(eq, eg, gg, dim - base < 64u ? dim - base : 64u, matches, cf, ce, stop);
        }
        if (stop) {
          if (lane == 0) { S.ex[at].EST_start = f.EST_start + (int)(cf - matches); S.ex[at].GEN_start = f.GEN_start + (int)(ce - matches); }
        } else {
          if (lane == 0) S.marks[at] |= 1u;
          ++lo;
        }
      } else {
        int j = (int)dim - 1, cf = (int)la - 1, ce = (int)lb - 1;
        uint32_t matches = 0;
        bool stop = false, done = false;
        while (!done) {
          const uint32_t wb = j >= 63 ? (uint32_t)j - 63u : 0u;            // lane t holds column wb + t
          const uint32_t col = wb + lane;
          const uint32_t xe = col < dim ? ea[col] : 0u, xg = col < dim ? ga[col] : 0u;
          const unsigned long long eq = __ballot(col < dim && xe == xg), eg = __ballot(xe == '-'), gg = __ballot(xg == '-');
          done = tail_walk_window(eq, eg, gg, wb, j, matches, cf, ce, stop);
        }
        int est_cl = cf + (int)matches, gen_cl = ce + (int)matches;
        MemRows rows{ea, ga};
        close_tail_gaps(rows, dim, (uint32_t)(j + (int)matches + 1), est_cl, gen_cl);
        if (gen_cl >= 0) {
          if (lane == 0) { S.ex[at].EST_end = f.EST_start + est_cl; S.ex[at].GEN_end = f.GEN_start + gen_cl; }
        } else {
          if (lane == 0) S.marks[at] |= 1u;
          --hi;
        }
      }
      __syncthreads();                                                      // the exon as trimmed, for every lane
      if (lo == hi) cr.verdict = 3;
    }
    // ---- step 3: clean_external_exons (:1706-1825)
    for (uint32_t end = 0; end < 2 && !refused && cr.verdict == 0; ++end) {
      const uint32_t at = end == 0 ? lo : hi - 1;
      const bool ok = external_exon_ok(T, n, est, S.ex, lo, hi, end, lane);
      if (!ok) {
        if (lane == 0) S.marks[at] |= 2u;
        if (end == 0) ++lo; else --hi;
        if (lo == hi) cr.verdict = 4;
      }
    }
    __syncthreads();
    // ---- step 4: clean_low_complexity_exons_2 (:1667-1704)
    if (!refused && cr.verdict == 0) {
      unsigned long long bad = 0ull;
      for (uint32_t i = lo; i < hi; ++i) {
        const pgpu_factor f = S.ex[i];
        if (f.GEN_start > f.GEN_end) continue;
        DevJob job;
        job.a = T + f.GEN_start; job.la = (uint32_t)(f.GEN_end - f.GEN_start + 1);
        job.b = est + f.EST_start; job.lb = f.EST_end >= f.EST_start ? (uint32_t)(f.EST_end - f.EST_start + 1) : 0u;
        const unsigned long long thr = (unsigned long long)__double_as_longlong(q.complexity_threshold);
        job.p0 = 0; job.p1 = (uint32_t)thr; job.p2 = (uint32_t)(thr >> 32); job.tail = 1;
        job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 1;
        const uint32_t fl = (uint32_t)__builtin_amdgcn_readfirstlane((int)dust_flags_wave(job, lane));
        if (fl) {
          bad |= 1ull << i;
          if (lane == 0) S.marks[i] |= (uint8_t)(fl << 2);
        }
      }
      best_run(S.ex, bad, lo, hi);
      if (lo == hi) cr.verdict = 5;
    }
    // ---- step 5: clean_noisy_exons (:1842-1898), only_internals = false
    if (!refused && cr.verdict == 0) {
      bool wide = false;
      if (lane >= lo && lane < hi) {
        const pgpu_factor f = S.ex[lane];
        wide = f.GEN_start <= f.GEN_end && max_edit_for_exon((uint32_t)(f.GEN_end - f.GEN_start + 1)) > MAX_KBAND;
      }
      refused = __any(wide);
    }
    if (!refused && cr.verdict == 0) {
      unsigned long long bad = 0ull;
      for (uint32_t i = lo; i < hi; ++i) {
        const pgpu_factor f = S.ex[i];
        bool ok = false;
        if (f.GEN_start <= f.GEN_end) {
          DevJob job;
          job.a = T + f.GEN_start; job.la = (uint32_t)(f.GEN_end - f.GEN_start + 1);
          job.b = est + f.EST_start; job.lb = f.EST_end >= f.EST_start ? (uint32_t)(f.EST_end - f.EST_start + 1) : 0u;
          job.p0 = max_edit_for_exon(job.la); job.p1 = job.p2 = job.tail = 0;
          job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 1;
          lev_wave_body<1, MODE_KBAND>(job, res, w, lane);
          own_stores_visible();
          ok = __builtin_amdgcn_readfirstlane(res->v[0]) != 0;
          own_stores_visible();                                            // read before the next exon's answer lands
        }
        if (!ok) {
          bad |= 1ull << i;
          if (lane == 0) S.marks[i] |= 16u;
        }
      }
      best_run(S.ex, bad, lo, hi);
      if (lo == hi) cr.verdict = 6;
    }
    // ---- step 6: check_est_coverage (:2303-2321)
    if (!refused && cr.verdict == 0) {
      const int cover = S.ex[hi - 1].EST_end - S.ex[lo].EST_start + 1;
      if (!((double)cover / (double)q.est_len >= (double)0.35f)) cr.verdict = 7;
    }
    __syncthreads();                                                        // the marks
    if (refused) { cr.status = PGPU_ERANGE; cr.verdict = 0; }
    else {
      if (cr.verdict == 0 || cr.verdict == 7) {
        cr.first_kept = lo; cr.n_kept = hi - lo;
        if (lane == 0) {
          out_exons[q.first_exon + lo].EST_start = S.ex[lo].EST_start; out_exons[q.first_exon + lo].GEN_start = S.ex[lo].GEN_start;
          out_exons[q.first_exon + hi - 1].EST_end = S.ex[hi - 1].EST_end; out_exons[q.first_exon + hi - 1].GEN_end = S.ex[hi - 1].GEN_end;
        }
      }
      if (lane < ne) out_marks[q.first_exon + lane] = S.marks[lane];
    }
    if (lane == 0) out[c] = cr;
  }
}

thread_local double t_clean_ms = 0.0;

constexpr size_t WS_BUDGET = (size_t)256 << 20;      // bytes of per-wave workspace a call allocates at the most (see the grid)

}  // namespace

// the grid: 16 waves per compute unit, fewer where one long end exon has made the workspace of a wave large (266 KB for
// 4096 genomic bytes under lev_wave<ALIGN>): the workspaces together stay within WS_BUDGET, at one wave per compute
// unit at the least, so that one such query costs the batch some parallelism and not an allocation of a gigabyte
hipError_t pgpu_clean_grid(size_t n, size_t ws_dirs, size_t ws_rows, size_t& waves, size_t& ws_wave) {
  ws_wave = (ws_dirs + ws_rows + sizeof(DevResult) + 255) & ~(size_t)255;      // as clean_kernel lays it out
  size_t cus = 0;
  const hipError_t e = chained_waves(n, waves, cus);
  if (e != hipSuccess) return e;
  if (waves * ws_wave > WS_BUDGET) {
    const size_t fit = WS_BUDGET / ws_wave > cus ? WS_BUDGET / ws_wave : cus;
    if (waves > fit) waves = fit;
  }
  return hipSuccess;
}

void pgpu_clean_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_clean_query* q,
                       uint32_t n, uint8_t* ws, size_t ws_dirs, size_t ws_rows, size_t waves, pgpu_factor* out_exons,
                       uint8_t* out_marks, pgpu_clean_result* out, uint32_t* undersized, hipStream_t st) {
  hipLaunchKernelGGL(clean_kernel, dim3((unsigned)waves), dim3(64), 0, st, T, tlen, ests, exons, q, n, ws, ws_dirs, ws_rows, out_exons,
                     out_marks, out, undersized);
}

extern "C" double pgpu_index_clean_chains_kernel_ms(void) { return t_clean_ms; }

extern "C" int pgpu_index_clean_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                       const pgpu_factor* exons, size_t n_exons_total, const pgpu_clean_query* q, size_t n,
                                       pgpu_factor* out_exons, uint8_t* out_marks, pgpu_clean_result* out) {
  t_clean_ms = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_clean_query) == 32 && sizeof(pgpu_clean_result) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  NamedExons named;
  const int begun = chained_begin(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_marks, out, "queries", named);
  if (begun != CHAINED_GO) return begun;
  const size_t glen = pgpu_index_length(idx);
  // the workspace of one wave holds the longest end-exon alignment of the call (trimming only shortens an exon)
  size_t ws_dirs = CLEAN_WS_DIRS_MIN, ws_rows = CLEAN_WS_ROWS_MIN;
  const auto own = [&](const pgpu_clean_query& x, const pgpu_factor* ex) {
    return clean_query_need(ex, x.n_exons, x.est_len, glen, ws_dirs, ws_rows);
  };
  if (!chained_queries_ok(q, n, ests_len, exons, n_exons_total, glen, named.p, own))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad clean query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two "
                                           "queries share, a coordinate outside what it indexes, or an end exon that begins in "
                                           "front of or ends behind its sequence)");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "clean chains");
  size_t waves = 0, ws_wave = 0;
  TRY_HIP(pgpu_clean_grid(n, ws_dirs, ws_rows, waves, ws_wave));
  const ChainedLayout L = chained_layout(ests_len, n_exons_total, n, sizeof *q, sizeof *out, 256, waves * ws_wave);
  TRY_HIP(hipMalloc((void**)&call.d, L.total));
  uint32_t* const d_undersized = (uint32_t*)(call.d + L.extra);      // the flag of a workspace sized too small, in the extra slot
  TRY_HIP(call.timing_events(1));
  TRY_HIP(chained_upload(call, L, ests, exons, q));
  TRY_HIP(hipMemsetAsync(d_undersized, 0, sizeof(uint32_t), call.st));
  TRY_HIP(call.record(0));
  pgpu_clean_launch(pgpu_index_genomic(idx), (uint32_t)glen, call.d, (const pgpu_factor*)(call.d + L.exons),
                    (const pgpu_clean_query*)(call.d + L.queries), (uint32_t)n, call.d + L.ws, ws_dirs, ws_rows, waves,
                    (pgpu_factor*)(call.d + L.out_exons), call.d + L.out_bytes, (pgpu_clean_result*)(call.d + L.results),
                    d_undersized, call.st);
  TRY_HIP(call.record(1));
  TRY_HIP(chained_download(call, L, out_exons, out_marks, out));
  uint32_t undersized = 0;
  TRY_HIP(hipMemcpyAsync(&undersized, d_undersized, sizeof undersized, hipMemcpyDeviceToHost, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  if (undersized) return pgpu_clean_undersized(ctx, "clean chains");
  call.elapsed_ms(0, &t_clean_ms);
  return PGPU_OK;
}
