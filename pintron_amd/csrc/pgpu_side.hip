// The side stage: from the MEG records of a unit's patterns (pgpu_meg.hip: every record ends with meg_write's text and the
// meg-edges.txt lines of its graph) to est-fact's three side files -- the entries of megs.txt and processed-megs.txt and
// the lines of meg-edges.txt of every settled unit, compact and in unit order.  processed-megs-info.txt holds per-EST
// microseconds and is not part of the stage.  Semantics: include/pintron_gpu.h (pgpu_unit_sides,
// pgpu_pairing_plan_run_sides).
//
// Two passes around three pgpu_exclusive_scan_u32 (megs, pmegs, edges):
//
//   side_count_kernel   one thread per unit, 256 per group: reads the unit's result and query, the header of one or two
//                       records and their two text lengths, the header and sequence lengths; sums the three texts in 64 bits,
//                       applies the cap, writes the verdict and the three u32 counts.  It guards everything the validator of
//                       the form without a plan refuses (a flagged record, lengths that pass the record's end, a pattern that
//                       is not there): such a unit is HOST, never a read outside an allocation.
//   side_write_kernel   one wave64 per unit, 4 waves per group; the wave of a unit that is not DONE leaves at once.  Lanes
//                       write the constant bytes (SEP, '>', '\n'); the wave copies every stretch through wave_copy
//                       (pgpu_wave_copy.h, shared with pgpu_text.hip): at most two H, S, M for megs, one of each for pmegs,
//                       H and X for edges.
//
// Why no aligned load of wave_copy leaves an allocation: a load may read up to 3 bytes before and past a stretch, inside
// the aligned words that hold its first and last byte.  Records begin at multiples of 4 of a blob whose base is a multiple
// of 256 and are padded to 4 bytes; M begins at a multiple of 4 inside its record (behind the graph part, itself padded,
// and 8 bytes of lengths) and X begins meg_text_len bytes later, at any residue, and ends in front of the record's padding:
// the words that hold the ends of M and X lie inside the record, so inside the record blob.  Headers and sequences are the
// stage's own copies (the plan's: the text stage's and the patterns'), which begin at multiples of 256 and have 16 bytes
// (TEXT_PAD; the plan's patterns: 64) behind them.
//
// LDS: 0 bytes.  No atomic and no fence: a unit's bytes belong to one wave.  No per-thread array, no stack frame.  The
// stage's one host wait is the last statement of pgpu_side_count (24 bytes: the three totals).
#include <stdlib.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_stage_drive.h"
#include "pgpu_side.h"
#include "pgpu_wave_copy.h"

namespace {

typedef unsigned long long u64;

// what both passes read
struct SideIn {
  const pgpu_unit_query* __restrict__ q; const pgpu_unit_result* __restrict__ units; uint32_t n;
  const uint8_t* __restrict__ recs; u64 recs_len; const u64* __restrict__ rec_first; uint32_t n_pat;
  const uint8_t* __restrict__ hdr; const u64* __restrict__ hdr_first;
  const uint8_t* __restrict__ seqs; const u64* __restrict__ seq_at; const u64* __restrict__ seq_off;
};

// what a pass needs of one pattern: its sequence and the two texts of its record; false: the pattern is not there, or its
// record is flagged or does not add up
struct PatView { const uint8_t* S; const uint8_t* M; u64 sl; uint32_t ml, xl; };
__device__ __forceinline__ bool pat_view(const SideIn& in, uint32_t x, PatView& v) {
  if (x >= in.n_pat) return false;
  const u64 a = in.rec_first[x], b = in.rec_first[x + 1];
  if ((a & 3u) || b < a || b > in.recs_len || b - a < 16u) return false;
  const u64 len = b - a;
  const uint8_t* const R = in.recs + a;
  const uint32_t* const h = (const uint32_t*)R;
  if (h[2] & (PGPU_MEG_TOO_COMPLEX | PGPU_MEG_UNAVAILABLE)) return false;
  const u64 graph = (16u + 12u * (u64)h[0] + 2u * ((u64)h[0] + 1u) + h[1] + 3u) & ~(u64)3u;
  if (graph + 8u > len) return false;
  const uint32_t* const t = (const uint32_t*)(R + graph);
  v.ml = t[0]; v.xl = t[1];
  if ((u64)v.ml + v.xl > len - graph - 8u) return false;
  v.M = R + graph + 8u;
  v.S = in.seqs + in.seq_at[x];
  v.sl = in.seq_off[x + 1] - in.seq_off[x];
  return true;
}

// what a pass needs of one settled unit: the forward pattern, the sibling on strand 1 (`two`), the header.  false: the
// unit is not one the rule covers, or names something that is not there.
struct UnitView { PatView f, r; bool two, aligned; u64 hl, h_at; };
__device__ __forceinline__ bool unit_view(const SideIn& in, const pgpu_unit_query& q, const pgpu_unit_result& o, uint32_t u,
                                          UnitView& v) {
  if (o.strand > 1u || (o.verdict != PGPU_UNIT_ALIGNED && o.verdict != PGPU_UNIT_UNALIGNED)) return false;
  v.two = o.strand == 1u; v.aligned = o.verdict == PGPU_UNIT_ALIGNED;
  if (v.two ? q.rev == PGPU_UNIT_NO_SIBLING : (!v.aligned && q.rev != PGPU_UNIT_NO_SIBLING)) return false;
  if (o.pattern != (v.two ? q.rev : q.fwd)) return false;
  if (!pat_view(in, q.fwd, v.f)) return false;
  if (v.two) { if (!pat_view(in, q.rev, v.r)) return false; }
  else v.r = v.f;
  v.h_at = in.hdr_first[u]; v.hl = in.hdr_first[u + 1] - v.h_at;
  return true;
}

// bytes of E(x) = ">" H "\n" S_x "\n" M_x
__device__ __forceinline__ u64 entry_len(u64 hl, const PatView& p) { return hl + p.sl + p.ml + 3u; }

__global__ __launch_bounds__(256)
void side_count_kernel(const SideIn in, pgpu_side_result* __restrict__ out, uint32_t* __restrict__ megs_counts,
                       uint32_t* __restrict__ pmegs_counts, uint32_t* __restrict__ edges_counts) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= in.n) return;
  const pgpu_unit_result o = in.units[u];
  pgpu_side_result r;
  r.megs_first = 0; r.pmegs_first = 0; r.edges_first = 0; r.megs_bytes = 0; r.pmegs_bytes = 0; r.edges_bytes = 0;
  r.verdict = PGPU_SIDE_NONE;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  if (o.verdict != PGPU_UNIT_HOST) {
    r.verdict = PGPU_SIDE_HOST;
    UnitView v;
    if (unit_view(in, in.q[u], o, u, v)) {
      const u64 megs = 15u + entry_len(v.hl, v.f) + (v.two ? 15u + entry_len(v.hl, v.r) : 0u);
      const u64 pmegs = v.aligned ? entry_len(v.hl, v.r) : 0u;        // v.r is the deciding pattern on either strand
      const u64 edges = v.aligned ? v.hl + 2u + v.r.xl : 0u;
      if (megs <= PGPU_SIDE_MAX_UNIT_BYTES && pmegs <= PGPU_SIDE_MAX_UNIT_BYTES && edges <= PGPU_SIDE_MAX_UNIT_BYTES) {
        r.verdict = PGPU_SIDE_DONE; r.megs_bytes = (uint32_t)megs; r.pmegs_bytes = (uint32_t)pmegs; r.edges_bytes = (uint32_t)edges;
      }
    }
  }
  out[u] = r;
  megs_counts[u] = r.megs_bytes;
  pmegs_counts[u] = r.pmegs_bytes;
  edges_counts[u] = r.edges_bytes;
}

// E(x) at p, by the whole wave; a DONE unit: every length is below 2^24
__device__ __forceinline__ uint8_t* put_entry(uint8_t* __restrict__ p, const uint8_t* __restrict__ H, uint32_t hl, const PatView& x,
                                              uint32_t lane) {
  const uint32_t sl = (uint32_t)x.sl;
  if (lane == 0) p[0] = '>';
  if (lane == 1) p[1u + hl] = '\n';
  if (lane == 2) p[2u + hl + sl] = '\n';
  wave_copy(p + 1, H, hl, lane);
  wave_copy(p + 2u + hl, x.S, sl, lane);
  wave_copy(p + 3u + hl + sl, x.M, x.ml, lane);
  return p + 3u + hl + sl + x.ml;
}
// SEP = "\n\n***********\n\n" at p
__device__ __forceinline__ uint8_t* put_sep(uint8_t* __restrict__ p, uint32_t lane) {
  if (lane < 15u) p[lane] = (lane < 2u || lane >= 13u) ? (uint8_t)'\n' : (uint8_t)'*';
  return p + 15;
}

__global__ __launch_bounds__(256)
void side_write_kernel(const SideIn in, pgpu_side_result* __restrict__ out, const u64* __restrict__ megs_first,
                       const u64* __restrict__ pmegs_first, const u64* __restrict__ edges_first, uint8_t* __restrict__ megs,
                       uint8_t* __restrict__ pmegs, uint8_t* __restrict__ edges) {
  const uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  if (u >= in.n) return;
  if (out[u].verdict != PGPU_SIDE_DONE) return;
  UnitView v;
  if (!unit_view(in, in.q[u], in.units[u], u, v)) return;     // (the count pass made such a unit HOST)
  const u64 megs_at = megs_first[u], pmegs_at = pmegs_first[u], edges_at = edges_first[u];
  if (lane == 0) { out[u].megs_first = megs_at; out[u].pmegs_first = pmegs_at; out[u].edges_first = edges_at; }
  const uint8_t* const H = in.hdr + v.h_at;
  const uint32_t hl = (uint32_t)v.hl;
  // megs(u) = SEP E(f) [SEP E(r)]
  uint8_t* p = put_entry(put_sep(megs + megs_at, lane), H, hl, v.f, lane);
  if (v.two) put_entry(put_sep(p, lane), H, hl, v.r, lane);
  if (!v.aligned) return;
  // pmegs(u) = E(the deciding pattern); edges(u) = ">" H "\n" X
  put_entry(pmegs + pmegs_at, H, hl, v.r, lane);
  uint8_t* const e = edges + edges_at;
  if (lane == 0) e[0] = '>';
  if (lane == 1) e[1u + hl] = '\n';
  wave_copy(e + 1, H, hl, lane);
  wave_copy(e + 2u + hl, v.r.M + v.r.ml, v.r.xl, lane);
}

SideIn side_in(const pgpu_side_job& d) {
  SideIn in;
  in.q = d.q; in.units = d.units; in.n = d.n;
  in.recs = d.recs; in.recs_len = d.recs_len; in.rec_first = d.rec_first; in.n_pat = d.n_pat;
  in.hdr = d.hdr; in.hdr_first = d.hdr_first;
  in.seqs = d.seqs; in.seq_at = d.seq_at; in.seq_off = d.seq_off;
  return in;
}

thread_local double t_side_ms = 0.0;

}  // namespace

hipError_t pgpu_side_count(pgpu_ctx* ctx, pgpu_side_job& d) {
  const uint32_t n = d.n;
  d.total[0] = d.total[1] = d.total[2] = 0;
  if (n == 0) return hipSuccess;                       // no kernel is ever launched with an empty grid
  const SideLayout L = side_layout(n, pgpu_scan_tmp_bytes((size_t)n + 1));
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  DRIVE(drive_record(d.ev, 0, st));
  hipLaunchKernelGGL(side_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, side_in(d), (pgpu_side_result*)(B + L.out),
                     (uint32_t*)(B + L.counts[0]), (uint32_t*)(B + L.counts[1]), (uint32_t*)(B + L.counts[2]));
  for (int k = 0; k < 3; ++k) DRIVE(drive_scan((uint32_t*)(B + L.counts[k]), (u64*)(B + L.first[k]), n, B + L.scan_tmp, st));
  for (int k = 0; k < 2; ++k)
    DRIVE(hipMemcpyAsync(&d.total[k], (const u64*)(B + L.first[k]) + n, sizeof d.total[k], hipMemcpyDeviceToHost, st));
  return drive_total(ctx, (const u64*)(B + L.first[2]), n, &d.total[2]);
}

hipError_t pgpu_side_write(pgpu_ctx* ctx, const pgpu_side_job& d, uint8_t* megs, uint8_t* pmegs, uint8_t* edges) {
  const uint32_t n = d.n;
  if (n == 0) return hipSuccess;
  const SideLayout L = side_layout(n, pgpu_scan_tmp_bytes((size_t)n + 1));
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  DRIVE(drive_record(d.ev, 2, st));
  hipLaunchKernelGGL(side_write_kernel, dim3((n + 3) / 4), dim3(256), 0, st, side_in(d), (pgpu_side_result*)(B + L.out),
                     (const u64*)(B + L.first[0]), (const u64*)(B + L.first[1]), (const u64*)(B + L.first[2]), megs, pmegs, edges);
  DRIVE(drive_record(d.ev, 1, st));
  return hipGetLastError();
}

// ---- the form without a plan -------------------------------------------------------------------------------------------
extern "C" double pgpu_unit_sides_kernel_ms(void) { return t_side_ms; }

extern "C" int pgpu_unit_sides(pgpu_ctx* ctx, const pgpu_unit_query* q, const pgpu_unit_result* units, size_t n,
                               const void* recs, size_t recs_len, const uint64_t* rec_first, size_t n_pat,
                               const char* headers, size_t headers_len, const uint64_t* hdr_first,
                               const char* seqs, size_t seqs_len, const uint64_t* seq_first,
                               pgpu_side_result* out, void* megs, size_t megs_cap, void* pmegs, size_t pmegs_cap,
                               void* edges, size_t edges_cap, size_t lens[3]) {
  t_side_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_side_result) == 40 && sizeof(pgpu_unit_result) == 24 && sizeof(pgpu_unit_query) == 16, "ABI layout");
  if (!ctx || !lens || !rec_first || !hdr_first || !seq_first || (n && (!q || !units || !out)) || (recs_len && !recs) ||
      (headers_len && !headers) || (seqs_len && !seqs) || (megs_cap && !megs) || (pmegs_cap && !pmegs) || (edges_cap && !edges))
    return PGPU_EINVAL;
  if (n > TEXT_MAX_COUNT || n_pat > TEXT_MAX_COUNT) return pgpu_ctx_fail(ctx, PGPU_EINVAL, TEXT_TOO_MANY);
  if (const char* wrong = side_records_wrong(rec_first, n_pat, recs_len)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (const char* wrong = text_offsets_wrong(hdr_first, n, headers_len, TEXT_BAD_HDR)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (const char* wrong = text_offsets_wrong(seq_first, n_pat, seqs_len, TEXT_BAD_SEQ)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (const char* wrong = side_units_wrong(q, units, n, recs, rec_first, n_pat)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  lens[0] = lens[1] = lens[2] = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "unit sides");
  // the one device block: [queries | units | records | their offsets | headers | their offsets | sequences | their offsets |
  // the stage's block]; the blobs follow in a second one, once the count pass has sized them
  const SideCallLayout C = side_call_layout(n, recs_len, n_pat, headers_len, seqs_len);
  const SideLayout L = side_layout(n, pgpu_scan_tmp_bytes(n + 1));
  TRY_HIP(hipMalloc((void**)&call.d, C.stage + L.total));
  TRY_HIP(call.timing_events(1));
  uint8_t* const B = call.d + C.stage;
  TRY_HIP(hipMemcpyAsync(call.d + C.q, q, n * sizeof *q, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + C.units, units, n * sizeof *units, hipMemcpyHostToDevice, call.st));
  if (recs_len) TRY_HIP(hipMemcpyAsync(call.d + C.recs, recs, recs_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + C.rec_first, rec_first, (n_pat + 1) * sizeof *rec_first, hipMemcpyHostToDevice, call.st));
  if (headers_len) TRY_HIP(hipMemcpyAsync(call.d + C.hdr, headers, headers_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + C.hdr_first, hdr_first, (n + 1) * sizeof *hdr_first, hipMemcpyHostToDevice, call.st));
  if (seqs_len) TRY_HIP(hipMemcpyAsync(call.d + C.seqs, seqs, seqs_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + C.seq_first, seq_first, (n_pat + 1) * sizeof *seq_first, hipMemcpyHostToDevice, call.st));
  pgpu_side_job job;
  job.q = (const pgpu_unit_query*)(call.d + C.q); job.units = (const pgpu_unit_result*)(call.d + C.units); job.n = (uint32_t)n;
  job.recs = call.d + C.recs; job.recs_len = recs_len; job.rec_first = (const u64*)(call.d + C.rec_first); job.n_pat = (uint32_t)n_pat;
  job.hdr = call.d + C.hdr; job.hdr_first = (const u64*)(call.d + C.hdr_first);
  job.seqs = call.d + C.seqs; job.seq_at = job.seq_off = (const u64*)(call.d + C.seq_first);
  job.block = B; job.ev[0] = call.ev[0]; job.ev[1] = call.ev[1]; job.ev[2] = nullptr;
  TRY_HIP(pgpu_side_count(ctx, job));
  for (int k = 0; k < 3; ++k) lens[k] = (size_t)job.total[k];
  if (job.total[0] > megs_cap || job.total[1] > pmegs_cap || job.total[2] > edges_cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, SIDE_NO_SPACE);
  const SideBlobs S = side_blobs(job.total);
  TRY_HIP(hipMalloc((void**)&call.d2, S.total));
  TRY_HIP(pgpu_side_write(ctx, job, call.d2 + S.at[0], call.d2 + S.at[1], call.d2 + S.at[2]));
  TRY_HIP(hipMemcpyAsync(out, B + L.out, n * sizeof *out, hipMemcpyDeviceToHost, call.st));
  void* const dst[3] = { megs, pmegs, edges };
  for (int k = 0; k < 3; ++k)
    if (job.total[k]) TRY_HIP(hipMemcpyAsync(dst[k], call.d2 + S.at[k], (size_t)job.total[k], hipMemcpyDeviceToHost, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_side_ms);
  return PGPU_OK;
}
