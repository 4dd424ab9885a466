// What the drives of the device stages share (pgpu_fact_drive, pgpu_final_drive, pgpu_unit_drive, pgpu_text_count,
// pgpu_side_count, pgpu_index_candidates, the plan's scan_total): DRIVE inside a function that returns hipError_t, and the compact tail.  Internal; host code only.
#pragma once
#include "pgpu_index.h"

#define DRIVE(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
// event k of a job: the array holds nulls when the context does not time its calls
inline hipError_t drive_record(const hipEvent_t* ev, int k, hipStream_t st) { return ev[k] ? hipEventRecord(ev[k], st) : hipSuccess; }
// behind the count pass, which wrote counts[0 .. n): counts[n] = 0, first[0 .. n] = the exclusive prefix sums of the n + 1
inline hipError_t drive_scan(uint32_t* counts, unsigned long long* first, size_t n, void* scan_tmp, hipStream_t st) {
  DRIVE(hipMemsetAsync(counts + n, 0, sizeof(uint32_t), st));
  pgpu_exclusive_scan_u32(counts, first, n + 1, scan_tmp, st);
  return hipSuccess;
}
// behind the write pass: first[n] into *total, the wait, and what a launch of the drive may have left behind
inline hipError_t drive_total(pgpu_ctx* ctx, const unsigned long long* first, size_t n, unsigned long long* total) {
  DRIVE(hipMemcpyAsync(total, first + n, sizeof *total, hipMemcpyDeviceToHost, pgpu_ctx_stream(ctx)));
  DRIVE(pgpu_ctx_wait(ctx));
  return hipGetLastError();
}
// The compact answer out of a drive's block (L: FactLayout or FinalLayout): the results, `res_bytes` in all, then the
// `total` exons and their step bytes when there are any.  The caller waits.
template <class Layout>
hipError_t drive_download(const uint8_t* block, const Layout& L, size_t res_bytes, unsigned long long total, void* out,
                          pgpu_factor* exons, uint8_t* steps, hipStream_t st) {
  DRIVE(hipMemcpyAsync(out, block + L.res, res_bytes, hipMemcpyDeviceToHost, st));
  if (!total) return hipSuccess;
  DRIVE(hipMemcpyAsync(exons, block + L.out_exons, (size_t)total * sizeof(pgpu_factor), hipMemcpyDeviceToHost, st));
  return hipMemcpyAsync(steps, block + L.out_steps, (size_t)total, hipMemcpyDeviceToHost, st);
}
