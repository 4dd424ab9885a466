// Intron classification and the small-exon search on the resident index.  Semantics: include/pintron_gpu.h; the
// device routines: pgpu_classify.h.
//
//   class_tables_kernel   one thread per position: the four 5' splice-site scores of an intron that starts there
//                         (GetScoreOf5Prime*BySS, src/classify-intron.c:231-330), the branch-point verdict of an
//                         intron that ends there (ExistsGoodBPS..., :535-618) and the two class bytes
//                         (pgpu_classify.h).  Once per index, on first use, kept until the index is destroyed.
//   classify_kernel       one thread per intron: pgpu_index_classify
//   small_exons_kernel    one wave per query: pgpu_index_small_exons
//
// Bit-exactness of the scores.  The reference is C99 on x86-64: every product and every sum of
// GetMatInspectorScoreOfaMotif (:620-663) is rounded on its own, and the classes hang on comparisons of the
// results (> 0.75, >= 0.75, > 0.25, u12 > u2).  The device therefore never multiplies and never calls log: the
// HOST computes, with the host's log and in the reference's order, W[k][base][i] = CV[k][i] * PWM[k][base][i] and
// the constant denominators sum_i CV[k][i] * MAXV[k][i], and uploads them; the device adds the selected entries
// in order (__dadd_rn: no contraction, no reassociation) and divides once (__ddiv_rn).
#include <math.h>
#include <string.h>

#include <new>

#include "pgpu_classify.h"
#include "pgpu_pwm_data.h"
#include "pgpu_query_call.h"

namespace {

struct PwmTables {
  double W[PGPU_N_PWM][4][PGPU_PWM_MAXLEN];
  double den[PGPU_N_PWM];
  int32_t len[PGPU_N_PWM];
};

// LoadPWMMatrices / GetCVectorForPWM / GetMAXVectorForPWM (:1498-1537) as ef_classify.c:59-73 restates them, then the
// products the motif score adds.  Products and sums must stay separate operations on the host as well: no
// contraction anywhere in this file.
#pragma clang fp contract(off)
void pwm_tables_fill(PwmTables* t) {
  const double* raw[PGPU_N_PWM] = { &pwm_raw_0[0][0], &pwm_raw_1[0][0], &pwm_raw_2[0][0], &pwm_raw_3[0][0], &pwm_raw_4[0][0], &pwm_raw_5[0][0] };
  memset(t, 0, sizeof *t);
  const double log5 = log((double)5.0f);          // the reference's log(5.0f) is C's double log; C++ would pick logf
  for (int k = 0; k < PGPU_N_PWM; ++k) {
    const int n = pwm_len[k];
    double pwm[4][PGPU_PWM_MAXLEN], cv[PGPU_PWM_MAXLEN], maxv[PGPU_PWM_MAXLEN];
    for (int b = 0; b < 4; ++b) for (int i = 0; i < n; ++i) pwm[b][i] = raw[k][b * n + i] + 0.00001f;
    for (int i = 0; i < n; ++i) {
      cv[i] = 0;
      for (int b = 0; b < 4; ++b) cv[i] += pwm[b][i] * log(pwm[b][i]);
      cv[i] += log5;
      cv[i] *= (100.0f / log5);
      maxv[i] = 0.0f;
      for (int b = 0; b < 4; ++b) if (pwm[b][i] > maxv[i]) maxv[i] = pwm[b][i];
    }
    double den = 0.0f;
    for (int i = 0; i < n; ++i) {
      for (int b = 0; b < 4; ++b) t->W[k][b][i] = cv[i] * pwm[b][i];
      den += cv[i] * maxv[i];
    }
    t->den[k] = den;
    t->len[k] = n;
  }
}

// row of a matrix for a byte: N counts as A (:633-650); -1 for every other byte (the reference indexes row -1 there;
// the motif then scores -1.0, as ef_classify.c:90-108)
__device__ __forceinline__ int pwm_row(uint32_t c) {
  switch (c) {
    case 'N': case 'n': case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
  }
  return -1;
}

// GetMatInspectorScoreOfaMotif over T[p .. p + len[k]); the caller guarantees that the window lies inside the sequence
__device__ __forceinline__ double motif_score(const PwmTables* __restrict__ pw, int k, const uint8_t* __restrict__ T, uint32_t p) {
  const int n = pw->len[k];
  double num = 0.0;
  bool bad = false;
  for (int i = 0; i < n; ++i) {
    const int r = pwm_row(T[p + i]);
    bad |= r < 0;
    num = __dadd_rn(num, pw->W[k][r < 0 ? 0 : r][i]);
  }
  return bad ? -1.0 : __ddiv_rn(num, pw->den[k]);
}

// the verdict of classify_genomic_intron_start_end's last lines (:191-210) for given scores
__device__ __forceinline__ uint32_t cmp_bits(double u12, double u2) {
  return (u12 > u2 ? 1u : 0u) | ((__dadd_rn(u12, -u2) > 0.25 && u12 >= 0.75) ? 2u : 0u);
}
__device__ __forceinline__ bool pair_is(const uint8_t* __restrict__ p, uint32_t a, uint32_t b) {
  return (p[0] == a && p[1] == b) || (p[0] == a + 32u && p[1] == b + 32u);
}

// one thread per position e in [0, n]; score5 = four tables of n + 1 doubles, one behind the other
__global__ __launch_bounds__(256)
void class_tables_kernel(const uint8_t* __restrict__ T, uint32_t n, const PwmTables* __restrict__ pw, double* __restrict__ score5,
                         uint8_t* __restrict__ cls_start, uint8_t* __restrict__ cls_end) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e > n) return;
  // the window of matrix k starts three bytes before the intron; real_substring clamps a negative start and cuts the
  // window at the end of the sequence, and a window that is short of the matrix scores -1.0 (its NUL is no base)
  double sc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t len = (uint32_t)pw->len[2 + k];
    sc[k] = (e < 3u || e - 3u + len > n) ? -1.0 : motif_score(pw, 2 + k, T, e - 3u);
    score5[(size_t)k * ((size_t)n + 1) + e] = sc[k];
  }
  uint32_t cs = 0x80u;
  {
    uint32_t kind = 0;
    if (e + 1u < n) kind = pair_is(T + e, 'G', 'T') ? CLS_P5_GT : pair_is(T + e, 'G', 'C') ? CLS_P5_GC : pair_is(T + e, 'A', 'T') ? CLS_P5_AT : 0u;
    const double m23 = sc[1] > sc[0] ? sc[1] : sc[0];              // u12 = s2, then "if (t > u12) u12 = t" with t = s3
    const double m45 = sc[3] > sc[2] ? sc[3] : sc[2];
    uint32_t own = 0;
    if (kind == CLS_P5_GT) own = cmp_bits(sc[0], sc[2]);
    else if (kind == CLS_P5_GC) own = cmp_bits(m23, sc[3]);
    else if (kind == CLS_P5_AT) own = cmp_bits(sc[1], m45);
    cs |= kind | (own << 2) | (cmp_bits(m23, m45) << 4);
  }
  cls_start[e] = (uint8_t)cs;
  // an intron whose last byte is T[e], at least 30 long: windows of 12 that start 30..14 bytes before its end E = e + 1,
  // all inside the intron; SearchBPS keeps the best score of each matrix and ExistsGoodBPS asks whether the better of
  // the two exceeds 0.75, i.e. whether any window of either matrix does
  uint32_t ce = 0;
  if (e >= 1u && e < n) {
    ce = 0x80u | (pair_is(T + e - 1, 'A', 'G') ? CLS_P3_AG : pair_is(T + e - 1, 'A', 'C') ? CLS_P3_AC : 0u);
    if (e + 1u >= 30u) {
      bool found = false;
      for (uint32_t i = 0; i <= 16u; ++i) {
        const uint32_t p = e + 1u - 30u + i;
        found |= motif_score(pw, 0, T, p) > 0.75 || motif_score(pw, 1, T, p) > 0.75;
      }
      if (found) ce |= 4u;
    }
  }
  cls_end[e] = (uint8_t)ce;
}

__global__ __launch_bounds__(256)
void classify_kernel(const ClassView cv, const pgpu_intron* __restrict__ in, uint32_t count, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) out[i] = (uint8_t)classify_intron(cv, in[i].start, in[i].end);
}

__global__ __launch_bounds__(64)
void small_exons_kernel(const LcfIndexView ix, const ClassView cv, const uint8_t* __restrict__ ests,
                        const pgpu_sexon_query* __restrict__ queries, pgpu_sexon_result* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  const pgpu_sexon_query q = queries[blockIdx.x];
  pgpu_sexon_result r;
  r.status = PGPU_OK; r.len = 0; r.offstart = 0; r.offend = 0; r.gpos = 0; r.i1type = 0; r.i2type = 0; r.pad = 0;
  if (q.elen > SEXON_MAX_ELEN) {
    r.status = PGPU_ERANGE;
  } else {
    const unsigned long long best = sexon_search(ix, cv, ests + q.e_off, q.elen, q.allgstart, q.allglen, q.f1slen, q.f2plen,
                                                 q.min_intron_len, lane);
    if (best) {
      r.len = sexon_key_len(best); r.offstart = sexon_key_offstart(best); r.gpos = sexon_key_occ(best);
      r.offend = q.elen - r.offstart - r.len;
      r.i1type = classify_intron(cv, q.allgstart + r.offstart, r.gpos - 1u);
      r.i2type = classify_intron(cv, r.gpos + r.len, q.allgstart + q.allglen - r.offend - 1u);
    }
  }
  if (lane == 0) out[blockIdx.x] = r;
}

// ---- the tables of an index ---------------------------------------------------------------------------------
struct ClassTables {
  double* d_score5 = nullptr;       // 4 x (n + 1)
  uint8_t* d_cls = nullptr;         // cls_start (n + 1), then cls_end (n + 1)
  PwmTables* d_pwm = nullptr;
  size_t n = 0;
};
void class_tables_release(void* p) {
  ClassTables* t = (ClassTables*)p;
  (void)hipFree(t->d_score5); (void)hipFree(t->d_cls); (void)hipFree(t->d_pwm);
  delete t;
}

// The tables of `idx`, built now when nobody has asked before.  The index's mutex makes the first use safe for two
// contexts at once: the second waits and finds the finished tables (the builder has waited for its stream before it
// publishes them, so they are complete for every other stream).
int class_tables_get(pgpu_ctx* ctx, const pgpu_index* idx, const ClassTables** out) {
  pgpu_index_lazy* slot = pgpu_index_lazy_slot(idx);
  std::lock_guard<std::mutex> lock(slot->mu);
  if (slot->tables) { *out = (const ClassTables*)slot->tables; return PGPU_OK; }
  ClassTables* t = new (std::nothrow) ClassTables();
  PwmTables* host = new (std::nothrow) PwmTables();
  if (!t || !host) { delete t; delete host; return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of host memory"); }
  pwm_tables_fill(host);
  t->n = pgpu_index_length(idx);
  const size_t n1 = t->n + 1;
  hipStream_t st = pgpu_ctx_stream(ctx);
  hipError_t e = hipMalloc((void**)&t->d_score5, 4 * n1 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_cls, 2 * n1);
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_pwm, sizeof(PwmTables));
  if (e == hipSuccess) e = hipMemcpyAsync(t->d_pwm, host, sizeof(PwmTables), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(class_tables_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, pgpu_index_genomic(idx),
                       (uint32_t)t->n, t->d_pwm, t->d_score5, t->d_cls, t->d_cls + n1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);       // also: `host` is read by the copy until here
  delete host;
  if (e != hipSuccess) {
    class_tables_release(t);
    return pgpu_ctx_fail(ctx, pgpu_code_of(e), hipGetErrorString(e));
  }
  slot->release = class_tables_release;
  slot->tables = t;
  *out = t;
  return PGPU_OK;
}

ClassView class_view(const ClassTables* t) {
  ClassView v; v.cls_start = t->d_cls; v.cls_end = t->d_cls + t->n + 1; v.n = (uint32_t)t->n;
  return v;
}

thread_local double t_sexon_ms = 0.0;

}  // namespace

int pgpu_class_view_get(pgpu_ctx* ctx, const pgpu_index* idx, ClassView* out) {
  const ClassTables* t = nullptr;
  const int rc = class_tables_get(ctx, idx, &t);
  if (rc == PGPU_OK) *out = class_view(t);
  return rc;
}

extern "C" double pgpu_index_small_exons_kernel_ms(void) { return t_sexon_ms; }

extern "C" int pgpu_index_classify(pgpu_ctx* ctx, const pgpu_index* idx, const pgpu_intron* introns, size_t n, uint8_t* out_type) {
  if (!ctx || !idx || (n && (!introns || !out_type))) return PGPU_EINVAL;
  if (n == 0) return PGPU_OK;
  if (n > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 introns in one call");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  const ClassTables* t = nullptr;
  int rc = class_tables_get(ctx, idx, &t);
  if (rc != PGPU_OK) return rc;
  QueryCall call(ctx, nullptr);                             // no range, no events
  const hipStream_t st = call.st;
  const size_t o_out = up256(n * sizeof(pgpu_intron));
  TRY_HIP(hipMalloc((void**)&call.d, o_out + up256(n)));
  TRY_HIP(hipMemcpyAsync(call.d, introns, n * sizeof(pgpu_intron), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(classify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, class_view(t),
                     (const pgpu_intron*)call.d, (uint32_t)n, call.d + o_out);
  TRY_HIP(hipMemcpyAsync(out_type, call.d + o_out, n, hipMemcpyDeviceToHost, st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  return PGPU_OK;
}

extern "C" int pgpu_index_score5(pgpu_ctx* ctx, const pgpu_index* idx, int k, double* out, size_t cap) {
  if (!ctx || !idx || !out || k < 0 || k > 3) return PGPU_EINVAL;
  const size_t n1 = pgpu_index_length(idx) + 1;
  if (cap < n1) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "score table buffer too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  const ClassTables* t = nullptr;
  int rc = class_tables_get(ctx, idx, &t);
  if (rc != PGPU_OK) return rc;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (hipMemcpyAsync(out, t->d_score5 + (size_t)k * n1, n1 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return pgpu_ctx_fail(ctx, PGPU_EDEVICE, "score table download failed");
  return PGPU_OK;
}

extern "C" int pgpu_index_small_exons(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                      const pgpu_sexon_query* q, size_t n, pgpu_sexon_result* out) {
  t_sexon_ms = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  if (!ctx || !idx || (n && (!q || !out)) || (ests_len && !ests)) return PGPU_EINVAL;
  if (n > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 queries in one call");
  const size_t glen = pgpu_index_length(idx);
  for (size_t i = 0; i < n; ++i) {
    if (q[i].reserved != 0 || q[i].min_intron_len < 4 || q[i].e_off > ests_len || q[i].elen > ests_len - q[i].e_off ||
        q[i].allgstart > glen || q[i].allglen > glen - q[i].allgstart)
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad small-exon query (reserved != 0, min_intron_len < 4, or efact / allgfact leave "
                                             "their sequence)");
  }
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  const ClassTables* t = nullptr;
  int rc = class_tables_get(ctx, idx, &t);
  if (rc != PGPU_OK) return rc;
  QueryCall call(ctx, "small_exons");
  const hipStream_t st = call.st;
  const size_t o_q = up256(ests_len + 64), o_r = o_q + up256(n * sizeof(pgpu_sexon_query)),
               total = o_r + up256(n * sizeof(pgpu_sexon_result));
  TRY_HIP(hipMalloc((void**)&call.d, total));
  TRY_HIP(call.timing_events(1));
  if (ests_len) TRY_HIP(hipMemcpyAsync(call.d, ests, ests_len, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(call.d + o_q, q, n * sizeof(pgpu_sexon_query), hipMemcpyHostToDevice, st));
  TRY_HIP(call.record(0));
  hipLaunchKernelGGL(small_exons_kernel, dim3((unsigned)n), dim3(64), 0, st, pgpu_index_lcf_view(idx), class_view(t), call.d,
                     (const pgpu_sexon_query*)(call.d + o_q), (pgpu_sexon_result*)(call.d + o_r));
  TRY_HIP(call.record(1));
  TRY_HIP(hipMemcpyAsync(out, call.d + o_r, n * sizeof(pgpu_sexon_result), hipMemcpyDeviceToHost, st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_sexon_ms);
  return PGPU_OK;
}
