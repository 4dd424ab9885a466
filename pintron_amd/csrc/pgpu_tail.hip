// What est-fact does to a factorization directly behind the refinement loop, chained, on the resident index.  Semantics:
// include/pintron_gpu.h (pgpu_index_tail_chains): one query is one factorization, and the answer is what
// correct_composition_tail, detect_polyA_signal (src/detect-polya.c:42-166), remove_invalid_factorizations,
// recover_lost_prefixes_and_suffixes and remove_false_small_exons (src/factorization-refinement.c:120-165, :959-1266) make of it.
//
//   tail_kernel     one wave per query (a workgroup is one wave); a wave that has finished a query takes the next one of
//                   its stride.  The exons sit in the wave's LDS, one lane loads one.  Step 1 compares 64 bytes per ballot.
//                   Steps 2 and 3 and the list edits of steps 4 and 5 are wave-uniform work on scalars.  The dynamic
//                   programs are the bodies of pgpu_wave_dp.h, unchanged, each at ONE call site and at the smallest
//                   rows-per-lane that holds its cap: lev_wave_body<4, AFFIX> (256 rows) for the lost prefix and the lost
//                   suffix, lev_wave_body<2, ED> (the shorter string on the rows: at most 100) for the three edit distances
//                   of an analysis, lev_wave_body<2, BORDERS> (128 rows) for its border refinement.  The prefix windows are
//                   read backwards from the exon: the wave writes the two reversed windows into LDS and hands the AFFIX body
//                   pointers to them.  A question the host code does not ask (equal first bytes, equal strings, an exon that
//                   is not analysed) runs no DP here either.  Everything that decides is uniform over the wave.
//                   LDS of a wave: the exons (64 x 16), the four row-minimum arrays of the BORDERS mode (4 x 129 words), the
//                   job's result (48), the step bytes (64) and the two reversed windows (256 + 304): 3 760 bytes, nothing
//                   in HBM beside the call's block.
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_tail.h"
#include "pgpu_stage_launch.h"

namespace {

constexpr uint32_t MAX_EXONS = PGPU_TAIL_MAX_EXONS;
constexpr uint32_t MAX_AFFIX = PGPU_TAIL_MAX_AFFIX;
constexpr uint32_t MAX_AFFIX_GEN = 304;             // (int)(1.17 * 256) = 299 genomic bytes of a prefix window, rounded up to 16
constexpr uint32_t MAX_WINDOW = PGPU_TAIL_MAX_SMALL_WINDOW;
constexpr uint32_t MAX_SMALL_GEN = PGPU_TAIL_MAX_SMALL_GEN;
constexpr int UB_MED_EXON = PGPU_TAIL_UB_MED_EXON;
constexpr int AFFIXES_LENGTH = PGPU_TAIL_AFFIXES_LENGTH;
static_assert(MAX_EXONS == 64, "one lane per exon");
static_assert(MAX_AFFIX == 4 * 64, "lev_wave_body<4, AFFIX>: four rows of the EST window per lane");
static_assert(MAX_WINDOW == 2 * 64, "lev_wave_body<2, BORDERS>: two rows of the pattern per lane");
static_assert(UB_MED_EXON <= 2 * 64, "lev_wave_body<2, ED>: the shorter string, at most the analysed exon, on the rows");
static_assert((uint32_t)(1.17 * MAX_AFFIX) <= MAX_AFFIX_GEN, "the genomic window of a prefix");

constexpr uint8_t STEP_PREFIX = 0x10, STEP_SUFFIX = 0x20, STEP_TAIL = 0x40;

struct TailLds {
  pgpu_factor ex[MAX_EXONS];                  // the query's exons as the steps leave them
  uint32_t rowmin[4 * (MAX_WINDOW + 1)];      // pre, pre_pos, suf, suf_pos of the analysis at hand
  DevResult res;                              // the answer of the DP at hand
  uint8_t steps[MAX_EXONS];
  uint8_t rev_e[MAX_AFFIX];                   // the lost prefix's two windows, reversed
  uint8_t rev_g[MAX_AFFIX_GEN];
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ bool is_a(uint8_t c) { return c == 'a' || c == 'A'; }

// detect_polyA_signal (src/detect-polya.c:73-166) with the tail exon's ends as step 1 left them; the loops as written.
// Returns polyA | polyadenil << 1.  Every lane walks the same bytes.
__device__ __forceinline__ uint32_t polyA_flags(const uint8_t* __restrict__ orig, const uint32_t el, const uint8_t* __restrict__ T,
                                                const uint32_t gl, const int est_end, const int gen_end) {
  const uint8_t* const cl = orig + (est_end + 1);
  const int cll = (int)el - est_end - 1;
  int i = 0, matches = 0;
  bool stop = false;
  while (i < cll && !stop) {
    if (is_a(cl[i])) { if (matches >= 8) stop = true; else { ++matches; ++i; } }
    else { if (matches >= 8) stop = true; else i = cll; }
  }
  bool polyadenil = false;
  if (stop) {
    i = gen_end - 39 > 0 ? gen_end - 39 : 0;
    while (i <= gen_end && !polyadenil) {
      if (is_a(T[i]) && (uint32_t)i + 6u <= gl) {        // a hexamer cut short by the sequence's end does not match
        const uint8_t c1 = T[i + 1], c2 = T[i + 2];
        const bool lower = T[i] == 'a';
        const uint8_t a = lower ? 'a' : 'A', t = lower ? 't' : 'T';
        polyadenil = (c1 == a || c1 == t) && c2 == t && T[i + 3] == a && T[i + 4] == a && T[i + 5] == a;
      }
      ++i;
    }
    i = gen_end - 9 > 0 ? gen_end - 9 : 0;
    matches = 0;
    while (i <= gen_end + 10 && stop && (uint32_t)i < gl) {
      if (matches >= 6) stop = false;
      else { if (is_a(T[i])) ++matches; else matches = 0; ++i; }
    }
    if (stop) {
      i = gen_end + 1;
      int count = 0;
      while (i <= gen_end + 10 && stop && (uint32_t)i < gl) {
        if (count >= 7) stop = false;
        else { if (is_a(T[i])) ++count; ++i; }
      }
    }
  }
  return (stop ? 1u : 0u) | (polyadenil ? 2u : 0u);
}

__global__ __launch_bounds__(64)
void tail_kernel(const uint8_t* __restrict__ T, const uint32_t gl, const uint8_t* __restrict__ ests,
                 const pgpu_factor* __restrict__ exons, const pgpu_tail_query* __restrict__ queries, uint32_t n_queries,
                 pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps, pgpu_tail_result* __restrict__ out) {
  __shared__ TailLds S;
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_queries; c += gridDim.x) {
    const pgpu_tail_query q = queries[c];
    const uint8_t* const est = ests + q.est_off;
    const uint8_t* const orig = ests + q.orig_off;
    const uint32_t el = q.est_len, ne = q.n_exons;
    bool refused = ne > MAX_EXONS;
    __syncthreads();                                           // the query before is done with the LDS
    if (!refused && lane < ne) { S.ex[lane] = exons[q.first_exon + lane]; S.steps[lane] = 0; }
    __syncthreads();
    uint32_t added = 0, flags = 0, verdict = 0, recovered = 0;
    if (!refused) {
      // ---- step 1, correct_composition_tail: 64 bytes per ballot
      const int te = uni(S.ex[ne - 1].EST_end), tg = uni(S.ex[ne - 1].GEN_end);
      uint32_t i = (uint32_t)te + 1u, j = (uint32_t)tg + 1u;
      for (;;) {
        const bool eq = i + lane < el && j + lane < gl && orig[i + lane] == T[j + lane];
        const unsigned long long differ = ~__ballot(eq);
        const uint32_t run = differ ? (uint32_t)__builtin_ctzll(differ) : 64u;
        i += run; j += run;
        if (run < 64u) break;
      }
      added = i - ((uint32_t)te + 1u);
      __syncthreads();
      if (lane == 0 && added) { S.ex[ne - 1].EST_end = te + (int)added; S.ex[ne - 1].GEN_end = tg + (int)added; }
      __syncthreads();
      // ---- step 2, detect_polyA_signal
      flags = (uint32_t)uni((int)polyA_flags(orig, el, T, gl, te + (int)added, tg + (int)added));
      // ---- step 3, remove_invalid_factorizations
      bool invalid = false;
      if (lane < ne) {
        const pgpu_factor f = S.ex[lane];
        invalid = f.EST_start > f.EST_end || f.GEN_start > f.GEN_end;
        if (lane + 1 < ne) invalid = invalid || f.EST_end >= S.ex[lane + 1].EST_start || f.GEN_end >= S.ex[lane + 1].GEN_start;
      }
      verdict = __any(invalid) ? 1u : 0u;
    }
    if (!refused && verdict == 0) {
      // ---- step 4, recover_lost_prefixes_and_suffixes: side 0 the prefix, side 1 the suffix; both windows are taken from
      // the exons as they are now (a prefix moves the first exon's starts, a suffix the last one's ends), then both applied
      const int f_es = uni(S.ex[0].EST_start), f_gs = uni(S.ex[0].GEN_start);
      const int l_ee = uni(S.ex[ne - 1].EST_end), l_ge = uni(S.ex[ne - 1].GEN_end);
      uint32_t pre_e = 0, pre_g = 0, suf_len = 0;
      bool ask_pre = false, ask_suf = false;
      if (f_es > 0 && f_gs > 0) {
        const int flen = f_es < f_gs ? f_es : f_gs;
        const int cap = (int)((1.0 + 0.17) * (double)flen);
        pre_e = (uint32_t)(f_es < cap ? f_es : cap); pre_g = (uint32_t)(f_gs < cap ? f_gs : cap);
        ask_pre = est[f_es - 1] != T[f_gs - 1];
      }
      if (el - (uint32_t)l_ee > 1u && gl - (uint32_t)l_ge > 1u) {
        const uint32_t re = el - (uint32_t)l_ee - 1u, rg = gl - (uint32_t)l_ge - 1u;
        suf_len = re < rg ? re : rg;
        ask_suf = est[l_ee] != T[l_ge];
      }
      refused = (ask_pre && pre_e > MAX_AFFIX) || (ask_suf && suf_len > MAX_AFFIX);
      if (!refused && ask_pre) {
        for (uint32_t k = lane; k < pre_e; k += 64) S.rev_e[k] = est[(uint32_t)f_es - 1u - k];
        for (uint32_t k = lane; k < pre_g; k += 64) S.rev_g[k] = T[(uint32_t)f_gs - 1u - k];
      }
      uint32_t pre_cut_e = 0, pre_cut_g = 0, suf_cut_e = 0, suf_cut_g = 0;
      for (int side = 0; side < 2 && !refused; ++side) {
        if (!(side ? ask_suf : ask_pre)) continue;
        DevJob job;
        job.a = side ? est + l_ee : (const uint8_t*)S.rev_e; job.la = side ? suf_len : pre_e;
        job.b = side ? T + l_ge : (const uint8_t*)S.rev_g; job.lb = side ? suf_len : pre_g;
        job.p0 = job.p1 = job.p2 = job.tail = 0;
        job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 4;
        __syncthreads();                                       // the reversed windows; the answer before has been read
        lev_wave_body<4, MODE_AFFIX>(job, &S.res, nullptr, lane);
        __syncthreads();                                       // lane 0's answer, for every lane
        if (uni(S.res.v[0])) {
          const uint32_t ce = (uint32_t)uni(S.res.v[1]), cg = (uint32_t)uni(S.res.v[2]);
          if (side) { suf_cut_e = ce; suf_cut_g = cg; } else { pre_cut_e = ce; pre_cut_g = cg; }
          recovered |= 1u << side;
        }
      }
      if (!refused && lane == 0) {
        if (recovered & 1u) { S.ex[0].EST_start = f_es - (int)pre_cut_e; S.ex[0].GEN_start = f_gs - (int)pre_cut_g; S.steps[0] |= STEP_PREFIX; }
        if (recovered & 2u) { S.ex[ne - 1].EST_end = l_ee + (int)suf_cut_e; S.ex[ne - 1].GEN_end = l_ge + (int)suf_cut_g; S.steps[ne - 1] |= STEP_SUFFIX; }
      }
      __syncthreads();
      // ---- step 5, remove_false_small_exons (:1095-1125) with analyze_possibly_small_exon (:960-1093) in its loop
      int prev = -1, curr = -1, next = 0;
      bool removed = false;
      while (!refused) {
        if (!removed) { prev = curr; curr = next; next = (uint32_t)next + 1u < ne ? next + 1 : -1; }
        removed = false;
        if (next < 0) break;
        if (prev < 0) continue;
        const int p_es = uni(S.ex[prev].EST_start), p_ee = uni(S.ex[prev].EST_end), p_gs = uni(S.ex[prev].GEN_start), p_ge = uni(S.ex[prev].GEN_end);
        const int c_es = uni(S.ex[curr].EST_start), c_ee = uni(S.ex[curr].EST_end), c_gs = uni(S.ex[curr].GEN_start), c_ge = uni(S.ex[curr].GEN_end);
        const int n_es = uni(S.ex[next].EST_start), n_ee = uni(S.ex[next].EST_end), n_gs = uni(S.ex[next].GEN_start), n_ge = uni(S.ex[next].GEN_end);
        const int elen = c_ee + 1 - c_es, glen = c_ge + 1 - c_gs;
        if (elen > UB_MED_EXON) continue;
        uint32_t outcome = 1;
        if (p_ge < c_gs && c_ge < n_gs) {                      // (else: an earlier merge with off_t1 > off_t2 lost the order)
          const int estart = p_es + 1 > p_ee + 1 - AFFIXES_LENGTH ? p_es + 1 : p_ee + 1 - AFFIXES_LENGTH;
          const int eend = n_ee < n_es + AFFIXES_LENGTH ? n_ee : n_es + AFFIXES_LENGTH;
          const int epreflen = p_ee + 1 - estart, esufflen = eend - n_es, allelen = eend - estart;
          const int gstart = p_gs + 1 > p_ge + 1 - AFFIXES_LENGTH ? p_gs + 1 : p_ge + 1 - AFFIXES_LENGTH;
          const int gend = n_ge < n_gs + AFFIXES_LENGTH ? n_ge : n_gs + AFFIXES_LENGTH;
          const int gpreflen = p_ge + 1 - gstart, gsufflen = gend - n_gs, allglen = gend - gstart;
          // the three edit distances (:990, :1012, :1017): 0 without a DP where the strings are equal
          const bool there2 = estart >= esufflen && gstart >= gsufflen;
          const uint8_t* const a0 = est + c_es; const uint8_t* const b0 = T + c_gs;
          const uint8_t* const a1 = est + estart; const uint8_t* const b1 = T + gstart;
          const uint8_t* const a2 = there2 ? est + (estart - esufflen) : est; const uint8_t* const b2 = there2 ? T + (gstart - gsufflen) : T;
          bool same0 = elen == glen, same1 = epreflen == gpreflen, same2 = esufflen == gsufflen;
          if (same0) for (int x = (int)lane; x < elen; x += 64) same0 = same0 && a0[x] == b0[x];
          if (same1) for (int x = (int)lane; x < epreflen; x += 64) same1 = same1 && a1[x] == b1[x];
          if (there2 && same2) for (int x = (int)lane; x < esufflen; x += 64) same2 = same2 && a2[x] == b2[x];
          const bool run0 = !__all(same0), run1 = !__all(same1), run2 = there2 && !__all(same2);
          refused = (uint32_t)allelen > MAX_WINDOW || (run0 && (uint32_t)glen > MAX_SMALL_GEN);
          if (refused) break;
          uint32_t max_errs = 0;
          for (int k = 0; k < 3; ++k) {
            if (!(k == 0 ? run0 : k == 1 ? run1 : run2)) continue;
            DevJob job;
            job.a = k == 0 ? a0 : k == 1 ? a1 : a2; job.la = (uint32_t)(k == 0 ? elen : k == 1 ? epreflen : esufflen);
            job.b = k == 0 ? b0 : k == 1 ? b1 : b2; job.lb = (uint32_t)(k == 0 ? glen : k == 1 ? gpreflen : gsufflen);
            job.p0 = job.p1 = job.p2 = job.tail = 0;
            job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 2;
            __syncthreads();                                   // the answer before has been read
            lev_wave_body<2, MODE_ED>(job, &S.res, nullptr, lane);
            __syncthreads();
            max_errs += (uint32_t)uni(S.res.v[0]);
          }
          DevJob job;
          job.a = est + estart; job.la = (uint32_t)allelen;
          job.b = T + gstart; job.lb = (uint32_t)allglen;
          job.p0 = 0; job.p1 = (uint32_t)allelen; job.p2 = max_errs;
          job.tail = gl - (uint32_t)gend >= 2u ? 2u : gl - (uint32_t)gend;
          job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 2;
          __syncthreads();
          lev_wave_body<2, MODE_BORDERS>(job, &S.res, nullptr, lane, S.rowmin);
          __syncthreads();
          if (uni(S.res.v[0])) {
            const int off_p = uni(S.res.v[1]), off_t1 = uni(S.res.v[2]), off_t2 = uni(S.res.v[3]);
            const int old2 = burset_adaptor(T, gl, (uint32_t)(p_ge + 1), (uint32_t)c_gs) + burset_adaptor(T, gl, (uint32_t)(c_ge + 1), (uint32_t)n_gs);
            const int nw = burset_adaptor(T, gl, (uint32_t)(gstart + off_t1), (uint32_t)(gstart + off_t2));
            outcome = 2 * nw >= old2 ? 3u : 2u;
            if (outcome == 3u && lane == 0) {                  // :1067-1070
              S.ex[prev].EST_end = estart + off_p - 1;
              S.ex[next].EST_start = eend + off_p - allelen;
              S.ex[prev].GEN_end = gstart + off_t1 - 1;
              S.ex[next].GEN_start = gend + off_t2 - allglen;
            }
          }
        }
        if (lane == 0) S.steps[curr] = (uint8_t)((S.steps[curr] & ~3u) | outcome);
        __syncthreads();
        if (outcome == 3u) {                                   // :1077-1083: curr is dropped, the merged prev is analysed again
          curr = prev;
          do { --prev; } while (prev >= 0 && (uni((int)S.steps[prev]) & 3) == 3);
          removed = true;
        }
      }
    }
    __syncthreads();
    pgpu_tail_result tr;
    tr.status = PGPU_OK; tr.verdict = (uint8_t)verdict; tr.polyA = (uint8_t)(flags & 1u); tr.polyadenil = (uint8_t)(flags >> 1);
    tr.recovered = 0; tr.n_kept = 0; tr.tail_added = added;
    if (refused) { tr.status = PGPU_ERANGE; tr.verdict = tr.polyA = tr.polyadenil = 0; tr.tail_added = 0; }
    else {
      const bool gone = verdict == 0 && lane < ne && (S.steps[lane] & 3u) == 3u;
      const uint32_t n_gone = (uint32_t)__popcll(__ballot(gone));
      if (verdict == 0) { tr.n_kept = ne - n_gone; tr.recovered = (uint8_t)recovered; }
      if (lane < ne) {
        out_exons[q.first_exon + lane] = S.ex[lane];
        uint8_t s = 0;
        if (verdict == 0) s = (uint8_t)(S.steps[lane] | (added && lane == ne - 1 ? STEP_TAIL : 0));
        out_steps[q.first_exon + lane] = s;
      }
    }
    if (lane == 0) out[c] = tr;
  }
}

thread_local double t_tail_ms = 0.0;

}  // namespace

void pgpu_tail_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_tail_query* q,
                      uint32_t n, size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out, hipStream_t st) {
  hipLaunchKernelGGL(tail_kernel, dim3((unsigned)waves), dim3(64), 0, st, T, tlen, ests, exons, q, n, out_exons, out_steps, out);
}

extern "C" double pgpu_index_tail_chains_kernel_ms(void) { return t_tail_ms; }

extern "C" int pgpu_index_tail_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                      const pgpu_factor* exons, size_t n_exons_total, const pgpu_tail_query* q, size_t n,
                                      pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out) {
  t_tail_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_tail_query) == 32 && sizeof(pgpu_tail_result) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  NamedExons named;
  const int begun = chained_begin(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_steps, out, "queries", named);
  if (begun != CHAINED_GO) return begun;
  const size_t glen = pgpu_index_length(idx);
  const auto own = [=](const pgpu_tail_query& x, const pgpu_factor* ex) { return tail_query_ok(x, ex, ests_len, glen); };
  if (!chained_queries_ok(q, n, ests_len, exons, n_exons_total, glen, named.p, own))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad tail query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two "
                                           "queries share, or a coordinate that is no byte of what it indexes)");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "tail chains");
  size_t waves = 0, cus = 0;
  TRY_HIP(chained_waves(n, waves, cus));
  const ChainedLayout L = chained_layout(ests_len, n_exons_total, n, sizeof *q, sizeof *out, 0, 0);
  TRY_HIP(hipMalloc((void**)&call.d, L.total));
  TRY_HIP(call.timing_events(1));
  TRY_HIP(chained_upload(call, L, ests, exons, q));
  TRY_HIP(call.record(0));
  pgpu_tail_launch(pgpu_index_genomic(idx), (uint32_t)glen, call.d, (const pgpu_factor*)(call.d + L.exons),
                   (const pgpu_tail_query*)(call.d + L.queries), (uint32_t)n, waves, (pgpu_factor*)(call.d + L.out_exons),
                   call.d + L.out_bytes, (pgpu_tail_result*)(call.d + L.results), call.st);
  TRY_HIP(call.record(1));
  TRY_HIP(chained_download(call, L, out_exons, out_steps, out));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_tail_ms);
  return PGPU_OK;
}
