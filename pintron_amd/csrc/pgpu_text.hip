// The text stage: from a unit's group in the packed records (pgpu_unit.hip) to est-fact's two text files -- the lines of
// raw-multifasta-out.txt and the entry of processed-ests.txt of every ALIGNED unit, compact and in unit order.
// Semantics: include/pintron_gpu.h (pgpu_unit_texts, pgpu_pairing_plan_run_texts).
//
// Two passes around two pgpu_exclusive_scan_u32 (raw and pests):
//
//   text_count_kernel   one thread per unit, 256 per group: walks the words of the unit's group and sums header length,
//                       constant strings, digit counts and clipped stretch lengths in 64 bits; writes the verdict and the
//                       two u32 counts.
//   text_write_kernel   one wave64 per unit, 4 waves per group; the wave of a unit that is not DONE leaves at once.  Lanes
//                       take the exons of a factorization, 64 at a time: each lane computes its line's length, a wave
//                       prefix sum (__shfl_up: no LDS) gives the line its offset, the lane writes its four numbers and
//                       separators in bytes (at most 50), and the wave then copies the stretches together, one after the
//                       other -- E and X of every exon, H per factorization, H and S of the pests entry -- through
//                       wave_copy.
//   wave_copy           (pgpu_wave_copy.h, shared with pgpu_side.hip) destination-aligned 4-byte stores by consecutive lanes; a source word is two aligned loads combined
//                       across the misalignment (__builtin_amdgcn_alignbyte), one when source and destination agree mod 4;
//                       single bytes only at the two edges (at most 3 each).  An aligned load may read up to 3 bytes before
//                       and past a stretch: headers, sequences and genomic lie in allocations whose base is a multiple of
//                       256 and have 16 bytes (TEXT_PAD; the plan's patterns: 64) behind them, so no load leaves one.
//
// LDS: 0 bytes.  No atomic and no fence: a unit's bytes belong to one wave.  No per-thread array, no stack frame.  The
// stage's one host wait is the last statement of pgpu_text_count (16 bytes: the two totals).
#include <stdlib.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_stage_drive.h"
#include "pgpu_text.h"
#include "pgpu_wave_copy.h"

namespace {

typedef unsigned long long u64;

// what both passes read
struct TextIn {
  const pgpu_unit_result* __restrict__ units; uint32_t n;
  const uint8_t* __restrict__ blob; u64 blob_len;
  const uint8_t* __restrict__ hdr; const u64* __restrict__ hdr_first;
  const uint8_t* __restrict__ seqs; const u64* __restrict__ seq_at; const u64* __restrict__ seq_off; uint32_t n_pat;
  const uint8_t* __restrict__ genomic; u64 gl;
};

__device__ __forceinline__ uint32_t digits_of(uint32_t a) {
  return 1u + (a >= 10u) + (a >= 100u) + (a >= 1000u) + (a >= 10000u) + (a >= 100000u) + (a >= 1000000u) + (a >= 10000000u) +
         (a >= 100000000u) + (a >= 1000000000u);
}
// bytes of printf("%d")
__device__ __forceinline__ uint32_t int_len(int32_t v) { return v < 0 ? 1u + digits_of(0u - (uint32_t)v) : digits_of((uint32_t)v); }
// printf("%d") at p; returns its bytes
__device__ __forceinline__ uint32_t put_int(uint8_t* __restrict__ p, int32_t v) {
  uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v, sign = 0;
  if (v < 0) { p[0] = '-'; sign = 1; }
  const uint32_t d = digits_of(a);
  for (uint32_t k = d; k-- > 0;) { p[sign + k] = (uint8_t)('0' + a % 10u); a /= 10u; }
  return sign + d;
}
// the stretch of a sequence of `len` bytes that the 1-based, inclusive [a, b] names: its length (it begins at a - 1)
__device__ __forceinline__ u64 clipped(int32_t a32, int32_t b32, u64 len) {
  const long long a = a32, b = b32;
  if (a < 1 || (u64)a > len + 1 || b < a) return 0;
  const u64 n = (u64)(b + 1 - a), rest = len - (u64)(a - 1);
  return n < rest ? n : rest;
}
// ">" H "\n#polya=" d "\n#polyad=" d "\n" without H: 1 + 8 + 9 + 1 and the two numbers
__device__ __forceinline__ uint32_t fact_head_len(uint32_t polya, uint32_t polyad) { return 19u + digits_of(polya) + digits_of(polyad); }
// byte j of "\n#polya=" d(polya) "\n#polyad=" d(polyad) "\n"
__device__ __forceinline__ uint8_t fact_tail_byte(uint32_t j, uint32_t polya, uint32_t polyad) {
  const uint32_t da = digits_of(polya), db = digits_of(polyad);
  if (j < 8u) return (uint8_t)"\n#polya="[j];
  j -= 8u;
  if (j < da) return (uint8_t)('0' + polya / (da - j == 3u ? 100u : da - j == 2u ? 10u : 1u) % 10u);
  j -= da;
  if (j < 9u) return (uint8_t)"\n#polyad="[j];
  j -= 9u;
  if (j < db) return (uint8_t)('0' + polyad / (db - j == 3u ? 100u : db - j == 2u ? 10u : 1u) % 10u);
  return (uint8_t)'\n';
}

// what a pass needs of one ALIGNED unit; false: the unit names something that is not there (a guard: the validator of the
// form without a plan and the unit driver hand no such unit in)
struct UnitView { const uint32_t* w; uint32_t n_words, n_fact; u64 hl, h_at, sl, s_at; };
__device__ __forceinline__ bool unit_view(const TextIn& in, const pgpu_unit_result& o, uint32_t u, UnitView& v) {
  if (o.pattern >= in.n_pat || ((o.first_byte | o.n_bytes) & 3u) || o.n_bytes < 8u || o.first_byte > in.blob_len ||
      o.n_bytes > in.blob_len - o.first_byte)
    return false;
  v.w = (const uint32_t*)(in.blob + o.first_byte);
  v.n_words = o.n_bytes >> 2; v.n_fact = v.w[1];
  v.h_at = in.hdr_first[u]; v.hl = in.hdr_first[u + 1] - v.h_at;
  v.s_at = in.seq_at[o.pattern]; v.sl = in.seq_off[o.pattern + 1] - in.seq_off[o.pattern];
  return true;
}

__global__ __launch_bounds__(256)
void text_count_kernel(const TextIn in, pgpu_text_result* __restrict__ out, uint32_t* __restrict__ raw_counts,
                       uint32_t* __restrict__ pests_counts) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= in.n) return;
  const pgpu_unit_result o = in.units[u];
  pgpu_text_result r;
  r.raw_first = 0; r.pests_first = 0; r.raw_bytes = 0; r.pests_bytes = 0; r.verdict = PGPU_TEXT_NONE;
  for (int k = 0; k < 7; ++k) r.reserved[k] = 0;
  UnitView v;
  if (o.verdict == PGPU_UNIT_ALIGNED) {
    r.verdict = PGPU_TEXT_HOST;
    if (unit_view(in, o, u, v)) {
      const u64 pests = v.hl + v.sl + 3u;
      u64 raw = 0;
      uint32_t at = 2;
      bool whole = true;
      for (uint32_t f = 0; f < v.n_fact && whole; ++f) {
        if (at >= v.n_words) { whole = false; break; }
        const uint32_t h = v.w[at], n_ex = h >> 16;
        ++at;
        if (n_ex > (v.n_words - at) >> 2) { whole = false; break; }
        raw += v.hl + fact_head_len(h & 0xffu, (h >> 8) & 0xffu);
        for (uint32_t k = 0; k < n_ex; ++k, at += 4) {
          const int32_t a = (int32_t)v.w[at], b = (int32_t)v.w[at + 1], c = (int32_t)v.w[at + 2], d = (int32_t)v.w[at + 3];
          raw += int_len(a) + int_len(b) + int_len(c) + int_len(d) + 6u + clipped(a, b, v.sl) + clipped(c, d, in.gl);
        }
      }
      if (whole && at == v.n_words && raw <= PGPU_TEXT_MAX_UNIT_BYTES && pests <= PGPU_TEXT_MAX_UNIT_BYTES) {
        r.verdict = PGPU_TEXT_DONE; r.raw_bytes = (uint32_t)raw; r.pests_bytes = (uint32_t)pests;
      }
    }
  }
  out[u] = r;
  raw_counts[u] = r.raw_bytes;
  pests_counts[u] = r.pests_bytes;
}

// lane k's value in every lane (k the same in all lanes)
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k); }

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(256)
void text_write_kernel(const TextIn in, pgpu_text_result* __restrict__ out, const u64* __restrict__ raw_first,
                       const u64* __restrict__ pests_first, uint8_t* __restrict__ raw, uint8_t* __restrict__ pests) {
  const uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  if (u >= in.n) return;
  if (out[u].verdict != PGPU_TEXT_DONE) return;
  const pgpu_unit_result o = in.units[u];
  UnitView v;
  if (!unit_view(in, o, u, v)) return;                 // (the count pass made such a unit HOST)
  const u64 raw_at = raw_first[u], pests_at = pests_first[u];
  if (lane == 0) { out[u].raw_first = raw_at; out[u].pests_first = pests_at; }
  const uint8_t* const H = in.hdr + v.h_at;
  const uint8_t* const S = in.seqs + v.s_at;
  const uint32_t hl = (uint32_t)v.hl, sl = (uint32_t)v.sl;        // a DONE unit: both below 2^24
  // pests(u) = ">" H "\n" S "\n"
  {
    uint8_t* const p = pests + pests_at;
    if (lane == 0) p[0] = '>';
    if (lane == 1) p[1 + hl] = '\n';
    if (lane == 2) p[2 + hl + sl] = '\n';
    wave_copy(p + 1, H, hl, lane);
    wave_copy(p + 2 + hl, S, sl, lane);
  }
  // raw(u)
  uint8_t* cur = raw + raw_at;
  uint32_t at = 2;
  const uint32_t n_fact = __builtin_amdgcn_readfirstlane(v.n_fact);
  for (uint32_t f = 0; f < n_fact; ++f) {
    const uint32_t h = __builtin_amdgcn_readfirstlane(v.w[at]), polya = h & 0xffu, polyad = (h >> 8) & 0xffu, n_ex = h >> 16;
    ++at;
    const uint32_t tail_len = fact_head_len(polya, polyad) - 1u;
    if (lane == 0) cur[0] = '>';
    if (lane < tail_len) cur[1 + hl + lane] = fact_tail_byte(lane, polya, polyad);
    wave_copy(cur + 1, H, hl, lane);
    cur += 1u + hl + tail_len;
    for (uint32_t base = 0; base < n_ex; base += 64) {
      const uint32_t cnt = n_ex - base < 64u ? n_ex - base : 64u;
      const bool have = lane < cnt;
      int32_t a = 0, b = 0, c = 0, d = 0;
      if (have) {
        const uint32_t* const x = v.w + at + 4u * (base + lane);
        a = (int32_t)x[0]; b = (int32_t)x[1]; c = (int32_t)x[2]; d = (int32_t)x[3];
      }
      const uint32_t le = have ? (uint32_t)clipped(a, b, v.sl) : 0u, lx = have ? (uint32_t)clipped(c, d, in.gl) : 0u;
      const uint32_t nums = int_len(a) + int_len(b) + int_len(c) + int_len(d) + 4u;      // the four numbers and their spaces
      const uint32_t line = have ? nums + le + lx + 2u : 0u;
      const uint32_t incl = wave_inclusive_sum(line, lane);
      const uint32_t off = incl - line;
      if (have) {
        uint8_t* p = cur + off;
        p += put_int(p, a); *p++ = ' ';
        p += put_int(p, b); *p++ = ' ';
        p += put_int(p, c); *p++ = ' ';
        p += put_int(p, d); *p++ = ' ';
        p[le] = ' ';
        p[le + 1u + lx] = '\n';
      }
      for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t e_at = lane_value(off + nums, k), le_k = lane_value(le, k), lx_k = lane_value(lx, k);
        const int32_t a_k = (int32_t)lane_value((uint32_t)a, k), c_k = (int32_t)lane_value((uint32_t)c, k);
        if (le_k) wave_copy(cur + e_at, S + (a_k - 1), le_k, lane);
        if (lx_k) wave_copy(cur + e_at + le_k + 1u, in.genomic + (c_k - 1), lx_k, lane);
      }
      cur += lane_value(incl, 63u);
    }
    at += 4u * n_ex;
  }
}

TextIn text_in(const pgpu_text_job& d, const TextLayout& L) {
  TextIn in;
  in.units = d.units; in.n = d.n; in.blob = d.blob; in.blob_len = d.blob_len;
  in.hdr = d.block + L.hdr; in.hdr_first = (const u64*)(d.block + L.hdr_first);
  in.seqs = d.seqs; in.seq_at = d.seq_at; in.seq_off = d.seq_off; in.n_pat = d.n_pat;
  in.genomic = d.genomic; in.gl = d.genomic_len;
  return in;
}

thread_local double t_text_ms = 0.0;

}  // namespace

hipError_t pgpu_text_count(pgpu_ctx* ctx, pgpu_text_job& d) {
  const uint32_t n = d.n;
  d.raw_total = d.pests_total = 0;
  if (n == 0) return hipSuccess;                       // no kernel is ever launched with an empty grid
  const TextLayout L = text_layout(n, d.headers_len, pgpu_scan_tmp_bytes((size_t)n + 1));
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  uint32_t* const raw_counts = (uint32_t*)(B + L.raw_counts);
  uint32_t* const pests_counts = (uint32_t*)(B + L.pests_counts);
  u64* const raw_first = (u64*)(B + L.raw_first);
  u64* const pests_first = (u64*)(B + L.pests_first);
  DRIVE(drive_record(d.ev, 0, st));
  hipLaunchKernelGGL(text_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, text_in(d, L), (pgpu_text_result*)(B + L.out),
                     raw_counts, pests_counts);
  DRIVE(drive_scan(raw_counts, raw_first, n, B + L.scan_tmp, st));
  DRIVE(drive_scan(pests_counts, pests_first, n, B + L.scan_tmp, st));
  DRIVE(hipMemcpyAsync(&d.raw_total, raw_first + n, sizeof d.raw_total, hipMemcpyDeviceToHost, st));
  return drive_total(ctx, pests_first, n, &d.pests_total);
}

hipError_t pgpu_text_write(pgpu_ctx* ctx, const pgpu_text_job& d, uint8_t* raw, uint8_t* pests) {
  const uint32_t n = d.n;
  if (n == 0) return hipSuccess;
  const TextLayout L = text_layout(n, d.headers_len, pgpu_scan_tmp_bytes((size_t)n + 1));
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  DRIVE(drive_record(d.ev, 2, st));
  hipLaunchKernelGGL(text_write_kernel, dim3((n + 3) / 4), dim3(256), 0, st, text_in(d, L), (pgpu_text_result*)(B + L.out),
                     (const u64*)(B + L.raw_first), (const u64*)(B + L.pests_first), raw, pests);
  DRIVE(drive_record(d.ev, 1, st));
  return hipGetLastError();
}

// ---- the genomic sequence ----------------------------------------------------------------------------------------------
extern "C" int pgpu_text_source_create(pgpu_ctx* ctx, const char* genomic_original, size_t len, pgpu_text_source** src) {
  if (!ctx || !src) return PGPU_EINVAL;
  *src = nullptr;
  if (!genomic_original || len == 0) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "a text source needs a genomic sequence");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  pgpu_text_source* s = (pgpu_text_source*)calloc(1, sizeof *s);
  if (!s) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of host memory");
  s->owner = ctx; s->len = len;
  hipError_t e = hipMalloc((void**)&s->d, len + TEXT_PAD);
  if (e == hipSuccess) e = hipMemsetAsync(s->d + len, 0, TEXT_PAD, pgpu_ctx_stream(ctx));
  if (e == hipSuccess) e = hipMemcpyAsync(s->d, genomic_original, len, hipMemcpyHostToDevice, pgpu_ctx_stream(ctx));
  if (e == hipSuccess) e = pgpu_ctx_wait(ctx);
  if (e != hipSuccess) {
    (void)hipFree(s->d); free(s);
    return pgpu_ctx_fail(ctx, pgpu_code_of(e), hipGetErrorString(e));
  }
  *src = s;
  return PGPU_OK;
}

extern "C" int pgpu_text_source_destroy(pgpu_ctx* ctx, pgpu_text_source* src) {
  if (!ctx || !src) return PGPU_EINVAL;
  if (src->owner != ctx) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "this text source was made on another context");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  (void)hipStreamSynchronize(pgpu_ctx_stream(ctx));
  (void)hipFree(src->d);
  free(src);
  return PGPU_OK;
}

// ---- the form without a plan -------------------------------------------------------------------------------------------
extern "C" double pgpu_unit_texts_kernel_ms(void) { return t_text_ms; }

extern "C" int pgpu_unit_texts(pgpu_ctx* ctx, const pgpu_unit_result* units, size_t n, const void* blob, size_t blob_len,
                               const char* headers, size_t headers_len, const uint64_t* hdr_first,
                               const char* seqs, size_t seqs_len, const uint64_t* seq_first, size_t n_pat,
                               const char* genomic, size_t genomic_len, pgpu_text_result* out,
                               void* raw, size_t raw_cap, size_t* raw_len, void* pests, size_t pests_cap, size_t* pests_len) {
  t_text_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_text_result) == 32 && sizeof(pgpu_unit_result) == 24, "ABI layout");
  if (!ctx || !raw_len || !pests_len || !hdr_first || !seq_first || (n && (!units || !out)) || (blob_len && !blob) ||
      (headers_len && !headers) || (seqs_len && !seqs) || (genomic_len && !genomic) || (raw_cap && !raw) || (pests_cap && !pests))
    return PGPU_EINVAL;
  if (n > TEXT_MAX_COUNT || n_pat > TEXT_MAX_COUNT) return pgpu_ctx_fail(ctx, PGPU_EINVAL, TEXT_TOO_MANY);
  if (const char* wrong = text_offsets_wrong(hdr_first, n, headers_len, TEXT_BAD_HDR)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (const char* wrong = text_offsets_wrong(seq_first, n_pat, seqs_len, TEXT_BAD_SEQ)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (const char* wrong = text_units_wrong(units, n, n_pat, blob, blob_len)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  *raw_len = 0; *pests_len = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "unit texts");
  // the one device block: [units | blob | sequences | their offsets | genomic | the stage's block]; the blobs follow in a
  // second one, once the count pass has sized them
  const TextCallLayout C = text_call_layout(n, blob_len, seqs_len, n_pat, genomic_len);
  const TextLayout L = text_layout(n, headers_len, pgpu_scan_tmp_bytes(n + 1));
  TRY_HIP(hipMalloc((void**)&call.d, C.stage + L.total));
  TRY_HIP(call.timing_events(1));
  uint8_t* const B = call.d + C.stage;
  TRY_HIP(hipMemcpyAsync(call.d + C.units, units, n * sizeof *units, hipMemcpyHostToDevice, call.st));
  if (blob_len) TRY_HIP(hipMemcpyAsync(call.d + C.blob, blob, blob_len, hipMemcpyHostToDevice, call.st));
  if (seqs_len) TRY_HIP(hipMemcpyAsync(call.d + C.seqs, seqs, seqs_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + C.seq_first, seq_first, (n_pat + 1) * sizeof *seq_first, hipMemcpyHostToDevice, call.st));
  if (genomic_len) TRY_HIP(hipMemcpyAsync(call.d + C.genomic, genomic, genomic_len, hipMemcpyHostToDevice, call.st));
  if (headers_len) TRY_HIP(hipMemcpyAsync(B + L.hdr, headers, headers_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(B + L.hdr_first, hdr_first, (n + 1) * sizeof *hdr_first, hipMemcpyHostToDevice, call.st));
  pgpu_text_job job;
  job.units = (const pgpu_unit_result*)(call.d + C.units); job.n = (uint32_t)n;
  job.blob = call.d + C.blob; job.blob_len = blob_len; job.headers_len = headers_len;
  job.seqs = call.d + C.seqs; job.seq_at = job.seq_off = (const u64*)(call.d + C.seq_first); job.n_pat = (uint32_t)n_pat;
  job.genomic = call.d + C.genomic; job.genomic_len = genomic_len;
  job.block = B; job.ev[0] = call.ev[0]; job.ev[1] = call.ev[1]; job.ev[2] = nullptr;
  TRY_HIP(pgpu_text_count(ctx, job));
  *raw_len = (size_t)job.raw_total; *pests_len = (size_t)job.pests_total;
  if (job.raw_total > raw_cap || job.pests_total > pests_cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "text buffers too small");
  const size_t o_pests = up256((size_t)job.raw_total ? (size_t)job.raw_total : 1);
  TRY_HIP(hipMalloc((void**)&call.d2, o_pests + up256((size_t)job.pests_total ? (size_t)job.pests_total : 1)));
  TRY_HIP(pgpu_text_write(ctx, job, call.d2, call.d2 + o_pests));
  TRY_HIP(hipMemcpyAsync(out, B + L.out, n * sizeof *out, hipMemcpyDeviceToHost, call.st));
  if (job.raw_total) TRY_HIP(hipMemcpyAsync(raw, call.d2, (size_t)job.raw_total, hipMemcpyDeviceToHost, call.st));
  if (job.pests_total) TRY_HIP(hipMemcpyAsync(pests, call.d2 + o_pests, (size_t)job.pests_total, hipMemcpyDeviceToHost, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_text_ms);
  return PGPU_OK;
}
