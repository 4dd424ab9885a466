// Internal declarations shared by the HIP translation units of libpintron_gpu.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_index.h"

// Job descriptor as the kernels see it: operand pointers already resolved to HBM addresses.
struct DevJob {
  const uint8_t* a;
  const uint8_t* b;
  uint32_t la, lb;
  uint32_t p0, p1, p2, tail;
  uint64_t ws_off;      // byte offset of this job's traceback workspace
  uint64_t str_off;     // byte offset of this job's two alignment strings
  uint32_t out_idx;     // index of the caller's job (results are written in caller order)
  uint32_t r_class;     // rows per lane (R) of the kernel instance that ran the job
};
static_assert(sizeof(DevJob) == 64, "DevJob layout");

using DevResult = pgpu_dp_result;

// kernel families: what the bodies of dp_batch_kernel's wave-per-job role are selected by (WaveSegs.family) and the
// first part of the sort key of the device job table
enum KernelFamily {
  KF_ALIGN = 0, KF_GAP, KF_ED, KF_KBAND, KF_LCF, KF_BORDERS, KF_AFFIX,
  KF_LCFSA,            // find_longest_common_factor_dp answered from the suffix array (one wave per job; see lcfsa_wave_body)
  KF_LCFW,             // ... of two short strings (the small-exon search's exon ends): one wave per job, a lane per diagonal
  KF_ALIGNB,           // ALIGN above 64 rows whose lengths differ by at most the band's half-width: inside the band on ONE
                       // wave (align_band_sweep); a job whose banded score exceeds the band is left with status
                       // ALIGN_BAND_RETRY and finished by the follow-up launch (launch_align_fallback) on four waves
  KF_COUNT
};

// row class of jobs with more than 4096 rows: run by the R = 64 kernels in strips of 4096 rows
constexpr uint32_t ROW_CLASS_STRIPS = 128;
constexpr int32_t ALIGN_BAND_RETRY = 1;     // DevResult.status of a banded ALIGN that has to be swept in full (never leaves the library)
constexpr uint32_t ALIGN_BAND_HALF = 31u;   // half-width of the band (2k + 1 <= 64 lanes)

// ---- the batch launch: ONE dp_batch_kernel for everything of a plan that is bound by the latency of its longest job ----
// Workgroups by index: [BORDERS on eight waves: bc][AFFIX on four: ac][ALIGN on four: lc][four wave-per-job jobs each];
// a wave of the last role finds its job in `segs` (family, first job, count; long-running families first).
// Both structs are the kernel's argument: their layout is fixed.
constexpr int MAX_WAVE_SEGS = 10;
struct WaveSegs { int n; int start[MAX_WAVE_SEGS]; int count[MAX_WAVE_SEGS]; int family[MAX_WAVE_SEGS]; };
struct BatchDesc { WaveSegs segs; int wave_blocks; int bc_start, bc_count, ac_start, ac_count, lc_start, lc_count; LcfIndexView ix; };
constexpr size_t DP_BATCH_MAX_LDS = 64 * 1024;       // the roles share one dynamic LDS array
// `wave_jobs`: there are wave-per-job workgroups; bc_max_rows: the longest BORDERS pattern (its row minima live in LDS)
size_t dp_batch_lds_bytes(bool wave_jobs, int bc_count, uint32_t bc_max_rows, int ac_count, int lc_count);
// false (nothing launched): the roles need more than DP_BATCH_MAX_LDS
bool launch_dp_batch(const DevJob* jobs, const BatchDesc& d, uint32_t bc_max_rows, DevResult* res, uint8_t* ws, uint8_t* strs,
                     hipStream_t st);
// behind it: the whole-matrix sweep (four waves per job) for the jobs of [jobs, jobs + njobs) the band could not settle
void launch_align_fallback(const DevJob* jobs, int njobs, DevResult* res, uint8_t* ws, uint8_t* strs, hipStream_t st);

// ---- launches of their own (pgpu_dp_kernels.hip): one launcher per stand-alone route of the plan builder's table ----
struct DpLaunch {
  const DevJob* jobs; int njobs;                        // the group's slice of the device job table
  uint32_t max_rows;                                    // largest a_len (BORDERS on eight waves: sizes the dynamic LDS)
  uint32_t max_chunks, max_l2;                          // LCF: most 256-diagonal chunks, longest s2
  DevResult* res; uint8_t* ws; uint8_t* strs;
  unsigned long long* keys;                             // LCF: the group's first key
  hipStream_t st;
};
using DpLauncher = void (*)(const DpLaunch&);
void launch_align_big(const DpLaunch& l);     // lev_any_kernel<ALIGN>: strips beyond 4096 rows, matrix + traceback
void launch_ed_big(const DpLaunch& l);        // lev_any_kernel<ED>: 32 / 64 rows per lane and strips
void launch_kband_big(const DpLaunch& l);     // lev_any_kernel<KBAND>: the same
void launch_gap_big(const DpLaunch& l);       // gap_any_kernel: 8 .. 32 rows per lane, + traceback
void launch_gap_slow(const DpLaunch& l);      // gap_slow_kernel: beyond 2048 rows
void launch_borders_coop(const DpLaunch& l);  // borders_coop_any_kernel: row minima beyond the batch launch's LDS
void launch_borders_slow(const DpLaunch& l);  // borders_slow_kernel: beyond 4096 rows
void launch_affix_strips(const DpLaunch& l);  // lev_wave_kernel<64, AFFIX, strips>: beyond 4096 rows
// keys: one zeroed entry per job, (length << 44) | (2^28-1 - occ1) << 16 | (2^16-1 - occ2) of the best run; 0: none
void launch_lcf(const DpLaunch& l);           // lcf_kernel; at most 65535 jobs (grid.y)

// ---- workspace layout shared by the plan builder and the kernels ----
// one boundary row (the last row of a strip, per column) in the job's workspace; there are two
__host__ __device__ inline size_t strip_bnd_bytes(uint32_t nc) { return (((size_t)nc + 1) * 4 + 15) & ~(size_t)15; }
// bytes of one traceback entry (all rows of one lane in one column): ALIGN on one wave and in strips, ...
static inline uint32_t align_entry_bytes(uint32_t R) { return R == ROW_CLASS_STRIPS ? 16u : (R <= 4 ? 1u : R / 4); }
// ... ALIGN with 65 .. 4096 rows on four waves (align_coop_body; rows per lane of the 256-lane sweep = r_class / 4), ...
static inline uint32_t align_coop_entry_bytes(uint32_t r_class) { const uint32_t R = r_class <= 4 ? 1u : r_class / 4; return R <= 4 ? 1u : R / 4; }
// ... GAP
static inline uint32_t gap_entry_bytes(uint32_t R) { return R; }
