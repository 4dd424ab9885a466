// Hand-written gfx950 (CDNA4, wave64) kernels for the est-fact dynamic programs.
//
// Common structure of the Levenshtein-family and gap kernels ("row strips x skewed column sweep"):
//   * one wavefront (64 lanes) owns one job; a 256-thread workgroup carries four independent jobs;
//   * lane l keeps R consecutive DP rows (l*R+1 .. l*R+R) of the CURRENT column in registers
//     (R is a template parameter: 1,2,4,...,64 -> up to 4096 rows);
//   * the wave sweeps the columns with a skew of one column per lane: at step s lane l works on
//     column s-l+1, so the anti-diagonal of strips is processed in parallel;
//   * the only inter-lane traffic per step is ONE 32-bit DPP wave shift (wave_shr:1) that hands
//     the value of the strip's last row -- packed with the column character, which therefore
//     travels down the lanes with the wavefront instead of being re-read -- to the lane below;
//   * traceback directions are packed (2 bits/cell, or 5 bits/cell for the 3-plane gap DP) and
//     stored step-major, [step][lane], so that every store instruction of the wave writes one
//     contiguous 64*entry-byte segment of HBM;
//   * tracebacks run in a second kernel, one wave per job: the chain of dependent direction
//     look-ups is walked in LDS (windows of the direction stream are staged there) with the walk
//     state in scalar registers, and the gapped strings are written by all lanes at once.
//
// Integer/character work only: no MFMA.  Reference routines are cited per kernel; paths are
// relative to the AlgoLab/PIntron tree.
#include "pgpu_internal.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_lcf.h"
#include <stdlib.h>

namespace {

// one row class per launch (AFFIX beyond 4096 rows, in strips)
template <int R, int MODE, bool STRIPS = false>
__global__ __launch_bounds__(256)
void lev_wave_kernel(const DevJob* __restrict__ jobs, int njobs, DevResult* __restrict__ results,
                     uint8_t* __restrict__ ws) {
  const uint32_t lane = threadIdx.x & 63u;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= njobs) return;
  const DevJob job = jobs[w];
  lev_wave_body<R, MODE, STRIPS>(job, &results[job.out_idx], ws, lane);
}

// ALL row classes of a family in ONE launch: the jobs of a batch are few per class, and
// kernels of one stream or hardware queue run one after the other, so a launch per class costs
// the sum of the classes' longest jobs; in one launch they overlap.  Every wave picks the body of
// its job's class (jobs are sorted by class, so the waves of a workgroup mostly agree).
// BIG = the classes with 32 and 64 rows per lane and the strips (rare in a batch, a few hundred
// registers per lane): they get a kernel of their own (lev_any_kernel), and the common classes up to
// 16 rows per lane run inside dp_batch_kernel, whose register budget lets several waves share a SIMD.
// Jobs are sorted big classes first, so the two take the two ends of the family's slice.
template <int MODE, bool BIG>
__device__ __forceinline__ void lev_any_dispatch(const DevJob& job, DevResult* res, uint8_t* __restrict__ ws, const uint32_t lane) {
  if constexpr (BIG) {
    switch (job.r_class) {
      case 32: lev_wave_body<32, MODE>(job, res, ws, lane); break;
      case 64: lev_wave_body<64, MODE>(job, res, ws, lane); break;
      default: lev_wave_body<64, MODE, true>(job, res, ws, lane); break;      // ROW_CLASS_STRIPS
    }
  } else {
    switch (job.r_class) {
      case 1:  lev_wave_body<1, MODE>(job, res, ws, lane); break;
      case 2:  lev_wave_body<2, MODE>(job, res, ws, lane); break;
      case 4:  lev_wave_body<4, MODE>(job, res, ws, lane); break;
      case 8:  lev_wave_body<8, MODE>(job, res, ws, lane); break;
      default: lev_wave_body<16, MODE>(job, res, ws, lane); break;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256)
void lev_any_kernel(const DevJob* __restrict__ jobs, int njobs, DevResult* __restrict__ results,
                    uint8_t* __restrict__ ws, uint8_t* __restrict__ strs) {
  const uint32_t lane = threadIdx.x & 63u;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= njobs) return;
  const DevJob job = jobs[w];
  DevResult* res = &results[job.out_idx];
  lev_any_dispatch<MODE, true>(job, res, ws, lane);
  if constexpr (MODE == MODE_ALIGN) {      // matrix, then the traceback by the same wave
    __shared__ __attribute__((aligned(16))) uint8_t s_win[4][TB_WIN_BYTES];
    __shared__ uint8_t s_path[4][TB_PATH];
    own_stores_visible();
    align_traceback_wave(job, res, ws, strs, lane, s_win[threadIdx.x >> 6], s_path[threadIdx.x >> 6]);
  }
}

// ---------------------------------------------------------------------------------------------
// Cooperative sweeps: one job over the W waves of a workgroup
// ---------------------------------------------------------------------------------------------
// A single wave needs (columns + 63) * R sequential cell updates for a job with 64*R rows; a merged
// batch holds only a few dozen jobs with hundreds of rows (small-exon searches, affix recovery),
// so those launches are latency-bound and sit on the critical path of every batch.  Here the
// strip of rows is spread over W*64 lanes: wave w owns lanes 64w .. 64w+63 of the same skewed
// sweep.  Lane 0 of wave w+1 needs, at step s, what lane 63 of wave w produced at step s-1; the
// waves are decoupled by one 64-step chunk: in interval k wave w works on chunk k-w and leaves the
// packed (value | column char) of its last lane, per step, in an LDS array that wave w+1 reads
// in the next interval (double-buffered; one __syncthreads per interval).  The column characters
// travel with the wavefront, so only wave 0 reads them from memory.
constexpr int COOP_W = 4;

template <int R, bool ROWMIN, bool AFFIX, bool ASMALL = false, bool WILD = false, bool DIRS = false>
__device__ __forceinline__ void lev_sweep_coop(const Operand rows, const uint32_t nr,
                                               const Operand cols, const uint32_t nc,
                                               const uint32_t w, const uint32_t lane,
                                               uint32_t* hand,        // [COOP_W-1][2][64] of this sweep
                                               uint32_t (&cur)[R], uint32_t (&minv)[R],
                                               uint32_t (&minpos)[R], AffixBest& best,
                                               uint8_t* dir_ws = nullptr) {   // DIRS: [step][256 lanes] entries
  uint32_t rc[R];
  const uint32_t gl = w * 64u + lane;   // lane index within the job (w is wave-uniform)
  const uint32_t row0 = gl * R;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = row0 + r;
    rc[r] = i < nr ? rows.at(i) : PAD_ROW;
    cur[r] = i + 1;
    if constexpr (ROWMIN) { minv[r] = i + 1; minpos[r] = 0; }
  }
  if (nr == 0 || nc == 0) return;       // uniform over the workgroup (one job)
  const uint32_t last_lane = (nr - 1) / R;
  const uint32_t steps = nc + last_lane;
  const uint32_t nchunks = (steps + 63u) / 64u;
  const bool wave_used = w * 64u <= last_lane;
  uint32_t diag_in = row0, out = 0;
  // The step loop is a chain of dependent instructions on one wave, so every instruction in it is
  // latency, and the hand-off between the waves costs ONE DPP move per step on either side:
  //  * producer: `hout` is a shift register, hout = (lanes move one down, lane 63 <- this step's
  //    `out` of lane 63); after the T steps of a chunk lane 63-k holds the step k before the last.
  //    It goes to the LDS array once per chunk (all lanes, one store);
  //  * consumer: reads the array once per chunk and turns it (one ds_bpermute) into `feed`, lane t =
  //    the input of step t = the producer's output of the step before; `feed` moves one lane down
  //    per step so lane 0 always holds the current input, and the DPP shift that passes the strips'
  //    last rows along drops it in.  Wave 0's feed is (top value | column character) instead.
  // No per-step LDS access, scalar round trip or branch on the wave number.  A wave's first cell
  // lies in chunk w; it looks at the array one chunk earlier for the step before its first.
  uint32_t hout = 0, prev = 0;
  uint32_t feed_next = (lane + 1u) | ((lane < nc ? cols.at(lane) : PAD_COL) << 24);   // wave 0: columns of chunk 0
  uint32_t* hand_in = hand + (w > 0 ? (w - 1) * 128u : 0u);
  uint32_t* hand_out = hand + (w + 1 < (uint32_t)COOP_W ? w : 0u) * 128u;

  for (uint32_t k = 0; k < nchunks + COOP_W - 1; ++k) {
    const int c = (int)k - (int)w;
    if (wave_used && w > 0 && c == (int)w - 1) prev = hand_in[(c & 1) * 64 + lane];
    if (wave_used && c >= (int)w && c < (int)nchunks) {
      const uint32_t s0 = (uint32_t)c * 64u;
      const uint32_t tmax = (min(64u, steps - s0) + 7u) & ~7u;   // whole groups of 8; steps past the end touch no cell
      uint32_t feed;
      if (w == 0) {
        feed = feed_next;                                    // requested one chunk ago (see lev_sweep)
        const uint32_t jn = s0 + 64u + lane;
        feed_next = (jn + 1u) | ((jn < nc ? cols.at(jn) : PAD_COL) << 24);
      } else {
        // the producer ran the same tmax steps on this chunk: its step t is in lane 64-tmax+t, the
        // last step of the chunk before in lane 63-tmax -- or, after a full chunk, in lane 63 of
        // what was read for the chunk before
        const uint32_t cur_in = hand_in[(c & 1) * 64 + lane];
        feed = (uint32_t)__shfl((int)cur_in, (int)((lane + 63u - tmax) & 63u));
        const uint32_t carry = (uint32_t)__builtin_amdgcn_readlane((int)prev, 63);
        if (tmax == 64u && lane == 0) feed = carry;
        prev = cur_in;
      }
      for (uint32_t t0 = 0; t0 < tmax; t0 += 8) {
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
          const uint32_t s = s0 + t0 + u;
          const uint32_t in = wave_shr1_first(feed, out);
          feed = wave_shl1(feed);
          const uint32_t j = s - gl + 1;
          if (j - 1u < nc) {
            const uint32_t ch = in >> 24;
            const uint32_t in_val = in & 0xFFFFFFu;
            uint32_t up = in_val;
            uint32_t diag = diag_in;
            const bool ch_n = WILD && is_n(ch);
            DirPack<R> dp;
            if constexpr (DIRS) dp.clear();
#pragma unroll
            for (int r = 0; r < R; ++r)
              lev_cell<R, WILD, DIRS, ROWMIN, AFFIX, false, ASMALL>(r, rc[r], ch, ch_n, diag, up, cur[r], minv[r], minpos[r], best, dp,
                                                                    row0 + r + 1, j, 0u);
            diag_in = in_val;
            out = up | (ch << 24);
            if constexpr (DIRS) dp.store(dir_ws + ((size_t)s * (64u * COOP_W) + gl) * (R <= 4 ? 1u : R / 4));
          }
          hout = wave_shl1_last(out, hout);
        }
      }
      if (w + 1 < (uint32_t)COOP_W) hand_out[(c & 1) * 64 + lane] = hout;
    }
    __syncthreads();
  }
}

// general_refine_borders (src/refine.c:105-192) for patterns longer than 64: the prefix sweep on
// waves 0-3 and the reversed-string sweep on waves 4-7 of one 512-thread workgroup.
template <int R>
__device__ __forceinline__ void borders_coop_body(const DevJob& job, DevResult* res) {
  extern __shared__ uint32_t lds[];      // hand-off [2][COOP_W-1][2][64], then the row minima (BordersMins)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // scalar: branches on it are uniform
  const uint32_t sweep = wave / COOP_W, w = wave % COOP_W;
  const uint32_t len_p = job.la, len_t = job.lb, max_errs = job.p2;
  const uint32_t t_win = min(len_p + max_errs, len_t);
  uint32_t* hand = lds + sweep * ((COOP_W - 1) * 128);
  const BordersMins mins{lds + 2 * (COOP_W - 1) * 128, len_p};
  uint32_t cur[R], minv[R], minpos[R];
  AffixBest best = AFFIX_NONE;
  const Operand rows{job.a, len_p, sweep == 1}, cols{job.b, len_t, sweep == 1};
  lev_sweep_coop<R, true, false>(rows, len_p, cols, t_win, w, lane, hand, cur, minv, minpos, best);
  uint32_t* mv = sweep ? mins.suf : mins.pre; uint32_t* mp = sweep ? mins.suf_pos : mins.pre_pos;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = (w * 64u + lane) * R + r + 1;
    if (i <= len_p) { mv[i] = minv[r]; mp[i] = minpos[r]; }
  }
  if (threadIdx.x == 0) { mins.pre[0] = 0; mins.pre_pos[0] = 0; mins.suf[0] = 0; mins.suf_pos[0] = 0; }
  __syncthreads();
  if (wave == 0) borders_cut_scan(job, res, lane, mins.pre, mins.pre_pos, mins.suf, mins.suf_pos);
}

// every row class above 64 rows in one launch (one job per workgroup; see lev_any_kernel)
__device__ __forceinline__ void borders_coop_dispatch(const DevJob& job, DevResult* res) {
  switch (job.r_class) {                 // rows per lane of the 256-lane sweep = class / COOP_W
    case 2: case 4: borders_coop_body<1>(job, res); break;
    case 8:  borders_coop_body<2>(job, res); break;
    case 16: borders_coop_body<4>(job, res); break;
    case 32: borders_coop_body<8>(job, res); break;
    default: borders_coop_body<16>(job, res); break;
  }
}

__global__ __launch_bounds__(512)
void borders_coop_any_kernel(const DevJob* __restrict__ jobs, int njobs, DevResult* __restrict__ results) {
  const DevJob job = jobs[blockIdx.x];
  borders_coop_dispatch(job, &results[job.out_idx]);
}

// find_longest_affix (src/factorization-refinement.c:1136-1173) for more than 64 rows
template <int R>
__device__ __forceinline__ void affix_coop_body(const DevJob& job, DevResult* res, uint32_t* hand, uint32_t (*wbest)[5]) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t cur[R], minv[R], minpos[R];
  AffixBest best = AFFIX_NONE;
  const Operand rows{job.a, 0, false}, cols{job.b, 0, false};
  // e + g < 2^15: every product of the cut test fits 24 x 24 -> 32 bits (AffixBest::consider)
  if (job.la + job.lb < 32768u) lev_sweep_coop<R, false, true, true>(rows, job.la, cols, job.lb, w, lane, hand, cur, minv, minpos, best);
  else                          lev_sweep_coop<R, false, true, false>(rows, job.la, cols, job.lb, w, lane, hand, cur, minv, minpos, best);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const AffixBest o = best.from_lane_xor(off);
    if (o.s && best.worse_than(o)) best = o;
  }
  if (lane == 0) { wbest[w][0] = best.v; wbest[w][1] = best.s; wbest[w][2] = best.e(); wbest[w][3] = best.g(); }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < COOP_W; ++k) {
      const AffixBest o{wbest[k][0], wbest[k][1], ((uint64_t)wbest[k][2] << 32) | wbest[k][3]};
      if (o.s && best.worse_than(o)) best = o;
    }
    res->status = 0; res->v[0] = (int32_t)best.valid();
    res->v[1] = (int32_t)best.e(); res->v[2] = (int32_t)best.g();
  }
}

__device__ __forceinline__ void affix_coop_dispatch(const DevJob& job, DevResult* res, uint32_t* hand, uint32_t (*wbest)[5]) {
  switch (job.r_class) {
    case 2: case 4: affix_coop_body<1>(job, res, hand, wbest); break;
    case 8:  affix_coop_body<2>(job, res, hand, wbest); break;
    case 16: affix_coop_body<4>(job, res, hand, wbest); break;
    case 32: affix_coop_body<8>(job, res, hand, wbest); break;
    default: affix_coop_body<16>(job, res, hand, wbest); break;
  }
}

// ---------------------------------------------------------------------------------------------
// ComputeAlignMatrix + TracebackAlignment (src/compute-alignments.c:85-207) for more than 64 rows: the sweep
// on the four waves of a workgroup (lev_sweep_coop with the N wildcard and the direction stream), the
// traceback by wave 0.  One wave needs rows/64 cells per step in a dependent chain (a 250-row exon: four
// cells per lane and step, 125 us); 256 lanes take one.  Directions are stored step-major over 256 lanes,
// [step][lane], 2 bits per row of the lane; the walk only ever needs the lanes at and below its own within a
// run of steps, so it stages a band of 64 lanes x (8192 / (64 x entry bytes)) steps in LDS.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t align_coop_rows_per_lane(uint32_t r_class) { return r_class <= 4u ? 1u : r_class / 4u; }

__device__ __forceinline__ void align_traceback_coop(const DevJob& job, DevResult* res, const uint8_t* __restrict__ ws,
                                                     uint8_t* __restrict__ strs, const uint32_t lane,
                                                     uint8_t* win, uint8_t* path) {
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.la), m = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.lb), cap = n + m + 1;
  uint8_t* ea = strs + job.str_off;
  uint8_t* ga = ea + cap;
  const uint32_t R = align_coop_rows_per_lane((uint32_t)__builtin_amdgcn_readfirstlane((int)job.r_class)), EB = R <= 4 ? 1u : R / 4;
  const uint32_t lgR = 31u - (uint32_t)__builtin_clz(R);
  const uint32_t WS = TB_WIN_BYTES / (64u * EB);           // sweep steps per window (band of 64 lanes)
  const uint8_t* dirs = ws + job.ws_off;
  const uint32_t LT = 64u * COOP_W;                        // lanes of the sweep
  uint32_t i = n, j = m, k = 0, np = 0;
  uint32_t i0 = n, j0 = m, pos = cap - 1;
  if (lane == 0) { ea[pos] = 0; ga[pos] = 0; }
  uint32_t s_lo = 1u, s_hi = 0u, g_lo = 0u;                // empty window
  while (i > 0 && j > 0) {
    const uint32_t gl = (i - 1) >> lgR, r = (i - 1) & (R - 1), s = (j - 1) + gl;
    if (s < s_lo || s > s_hi || gl < g_lo || gl >= g_lo + 64u) {
      // steps (s - WS, s], lanes [g_lo, g_lo + 64) with g_lo a multiple of 16 at least 32 below gl
      s_hi = s; s_lo = s + 1 >= WS ? s + 1 - WS : 0;
      g_lo = (gl & ~15u) >= 48u ? (gl & ~15u) - 48u : 0u;
      const uint32_t row16 = 4u * EB;                      // 16-byte pieces per step row of the band
      const uint32_t total16 = (s_hi - s_lo + 1) * row16;
      for (uint32_t e = lane; e < total16; e += 64u) {
        const uint32_t row = e / row16, c16 = e % row16;
        *reinterpret_cast<uint4*>(win + (size_t)e * 16u) =
            *reinterpret_cast<const uint4*>(dirs + ((size_t)(s_lo + row) * LT + g_lo) * EB + c16 * 16u);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    uint32_t d = (win[((s - s_lo) * 64u + (gl - g_lo)) * EB + (r >> 2)] >> (2u * (r & 3u))) & 3u;
    d = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
    path[np] = (uint8_t)d;                                // every lane, same address, same value: no exec games
    ++np;
    i -= d < 2u ? 1u : 0u;                                 // 0: diagonal, 1: up, 2: left -- no branches in the step
    j -= d != 1u ? 1u : 0u;
    if (np == TB_PATH) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      tb_flush(path, np, job.a, job.b, i0, j0, pos, ea, ga, lane);
      pos -= np; k += np; np = 0; i0 = i; j0 = j;
      __builtin_amdgcn_wave_barrier();
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  tb_flush(path, np, job.a, job.b, i0, j0, pos, ea, ga, lane);
  pos -= np; k += np;
  for (uint32_t q = lane; q < i; q += 64) { ea[pos - 1 - q] = job.a[i - 1 - q]; ga[pos - 1 - q] = '-'; }
  pos -= i; k += i;
  for (uint32_t q = lane; q < j; q += 64) { ea[pos - 1 - q] = '-'; ga[pos - 1 - q] = job.b[j - 1 - q]; }
  pos -= j; k += j;
  if (lane == 0) {
    res->v[1] = (int32_t)k;
    res->str[0] = job.str_off + pos;
    res->str[1] = job.str_off + cap + pos;
  }
}

// one job on the first four waves of a workgroup; smem: hand-off (3 x 128 words), then the traceback's
// window (TB_WIN_BYTES, 16-aligned) and path (TB_PATH)
constexpr size_t ALIGN_COOP_LDS = (COOP_W - 1) * 128 * sizeof(uint32_t) + TB_WIN_BYTES + TB_PATH;
template <int R>
__device__ __forceinline__ void align_coop_body(const DevJob& job, DevResult* res, uint8_t* __restrict__ ws,
                                                uint8_t* __restrict__ strs, uint8_t* smem) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* hand = reinterpret_cast<uint32_t*>(smem);
  uint8_t* win = smem + (COOP_W - 1) * 128 * sizeof(uint32_t);
  uint8_t* path = win + TB_WIN_BYTES;
  const uint32_t n = job.la, m = job.lb;
  // identity alignment, score 0 (compute-alignments.c:48-58)
  bool same = n == m;
  if (same) for (uint32_t q = threadIdx.x; q < n; q += 64u * COOP_W) same = same && job.a[q] == job.b[q];
  if (__syncthreads_and(same ? 1 : 0)) {
    if (w != 0) return;
    if (lane == 0) { res->status = 0; res->v[0] = 0; res->v[1] = (int32_t)n; res->v[5] = 1; }
    own_stores_visible();
    align_traceback_wave(job, res, ws, strs, lane, win, path);      // its identity branch
    return;
  }
  uint32_t cur[R], minv[R], minpos[R];
  AffixBest best = AFFIX_NONE;
  const Operand rows{job.a, 0, false}, cols{job.b, 0, false};
  lev_sweep_coop<R, false, false, false, true, true>(rows, n, cols, m, w, lane, hand, cur, minv, minpos, best, ws + job.ws_off);
  if (n == 0 || m == 0) { if (threadIdx.x == 0) { res->status = 0; res->v[0] = (int32_t)(n + m); res->v[5] = 0; } }
  else {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if ((w * 64u + lane) * R + r + 1 == n) { res->status = 0; res->v[0] = (int32_t)cur[r]; res->v[5] = 0; }
  }
  // the four waves' directions (and the score) have to be visible to wave 0
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (w != 0) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  align_traceback_coop(job, res, ws, strs, lane, win, path);
}

__device__ __forceinline__ void align_coop_dispatch(const DevJob& job, DevResult* res, uint8_t* __restrict__ ws,
                                                    uint8_t* __restrict__ strs, uint8_t* smem) {
  switch (job.r_class) {                 // rows per lane of the 256-lane sweep = class / COOP_W
    case 2: case 4: align_coop_body<1>(job, res, ws, strs, smem); break;
    case 8:  align_coop_body<2>(job, res, ws, strs, smem); break;
    case 16: align_coop_body<4>(job, res, ws, strs, smem); break;
    case 32: align_coop_body<8>(job, res, ws, strs, smem); break;
    default: align_coop_body<16>(job, res, ws, strs, smem); break;
  }
}

// the large row classes of a batch's gap alignments in one launch (see lev_any_kernel): 8 rows per lane
// and more (gap alignments of more than 256 EST characters: rare); the others run inside dp_batch_kernel
__global__ __launch_bounds__(256)
void gap_any_kernel(const DevJob* __restrict__ jobs, int njobs, DevResult* __restrict__ results,
                    uint8_t* __restrict__ ws, uint8_t* __restrict__ strs) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[4][TB_WIN_BYTES];
  __shared__ uint8_t s_path[4][TB_PATH];
  const uint32_t lane = threadIdx.x & 63u;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= njobs) return;
  const DevJob job = jobs[w];
  DevResult* res = &results[job.out_idx];
  switch (job.r_class) {
    case 8:  gap_wave_body<8>(job, res, ws, lane); break;
    case 16: gap_wave_body<16>(job, res, ws, lane); break;
    default: gap_wave_body<32>(job, res, ws, lane); break;
  }
  own_stores_visible();                  // the planes and the start plane (res->pad)
  gap_traceback_wave(job, res, ws, strs, lane, s_win[threadIdx.x >> 6], s_path[threadIdx.x >> 6]);
}

// (find_longest_common_factor_dp by one wave -- lcf_small_wave_body, lcfsa_wave_key, lcfsa_wave_body -- and lcf_key:
// pgpu_lcf.h, which pgpu_small.hip includes too)

// ---------------------------------------------------------------------------------------------
// End-exon alignments (ALIGN jobs with p0 = 1: first exon, p0 = 2: last exon; p1 / p2 = the complexity threshold's
// double bits).  handle_endpoints (src/est-factorizations.c:2127-2301) trims the exon by what the alignment shows at
// its outer end, and the next thing the host asks is the exon check of the TRIMMED exon (KBAND with tail = 1).  The
// wave that just wrote the alignment does both ahead of the host: it walks the outer 64 columns the way the host
// will, takes the trimmed exon as sub-operands and runs the exon check on them.  The answer comes back in the spare
// fields of the ALIGN result TOGETHER with the sub-operands it was computed for (v[2], v[3]: head -- characters of a
// and of b trimmed away; tail -- characters of a and of b kept) and the bound it used; the host files it under the
// question those define and finds it only if its own trimming -- done on the strings, as before -- asks exactly that
// question: a slip in this walk costs a second request, never a different result.  v[4] = ok | dust flags << 1 |
// valid << 3 | bound << 8.  Not attempted (valid = 0): the walk leaves the 64 columns, the exon is dropped, or the
// banded distance would need more than one row per lane.
// ---------------------------------------------------------------------------------------------
// (forceinline: as a call it gave dp_batch_kernel a stack frame -- 96 B of scratch per lane, 114 VGPRs -- and the kernel
// then wrote three times the bytes for the SAME jobs with no such job among them: PMC WRITE_SIZE of dp_batch_kernel over
// 20 000 C3 ESTs 778 -> 2 207 MiB, `tools/pmc_write_ab.sh` over the builds before and after; inlined: 106 VGPRs, no scratch)
__device__ __forceinline__ void endpoint_epilogue(const DevJob& job, DevResult* res, const uint8_t* __restrict__ strs,
                                               uint8_t* __restrict__ ws, const uint32_t lane, DevResult* tmp) {
  const uint32_t n = job.la, m = job.lb;
  const uint32_t dim = (uint32_t)__builtin_amdgcn_readfirstlane(res->v[1]);
  const uint8_t* ea = strs + res->str[0];
  const uint8_t* ga = strs + res->str[1];
  if (dim == 0u) return;
  uint32_t sub_a_off = 0, sub_b_off = 0, sub_la = 0, sub_lb = 0;
  bool valid = false;
  if (job.p0 == 1u) {
    // head (:2163-2196): columns from the left until more than five matches in a row
    const uint32_t c = lane < dim ? lane : dim;
    const uint32_t xe = lane < dim ? ea[c] : 0u, xg = lane < dim ? ga[c] : 0u;
    const unsigned long long eq = __ballot(lane < dim && xe == xg), eg = __ballot(xe == '-'), gg = __ballot(xg == '-');
    uint32_t matches = 0, cf = 0, ce = 0;
    bool stop = false;
    head_walk_window(eq, eg, gg, dim < 64u ? dim : 64u, matches, cf, ce, stop);
    if (stop && cf - matches <= n && ce - matches <= m) {       // (not stopped: the exon is dropped, or the walk goes on beyond the window)
      sub_a_off = cf - matches; sub_b_off = ce - matches; sub_la = n - sub_a_off; sub_lb = m - sub_b_off;
      valid = true;
    }
  } else {
    // tail (:2231-2296): columns from the right until more than ten matches in a row, then the gap columns next to
    // that run are closed by pulling the next character over, as far as the characters agree
    const uint32_t wb = dim > 64u ? dim - 64u : 0u;             // lane t holds column wb + t
    const uint32_t col = wb + lane;
    uint32_t xe = col < dim ? ea[col] : 0u, xg = col < dim ? ga[col] : 0u;
    const unsigned long long eq = __ballot(col < dim && xe == xg), eg = __ballot(xe == '-'), gg = __ballot(xg == '-');
    int j = (int)dim - 1, cf = (int)n - 1, ce = (int)m - 1;
    uint32_t matches = 0;
    bool stop = false;
    if (tail_walk_window(eq, eg, gg, wb, j, matches, cf, ce, stop)) {        // (false: the walk goes on beyond the window)
      int est_cl = cf + (int)matches, gen_cl = ce + (int)matches;
      // the window's columns in the lanes' registers; a NUL behind the row, as in the host's zero-padded copy
      struct LaneRows {
        uint32_t xe, xg; const uint32_t col, wb, dim;
        __device__ __forceinline__ uint32_t at(uint32_t v, uint32_t q) const { return q < dim ? (uint32_t)__shfl((int)v, (int)(q - wb)) : 0u; }
        __device__ __forceinline__ uint32_t e(uint32_t q) const { return at(xe, q); }
        __device__ __forceinline__ uint32_t g(uint32_t q) const { return at(xg, q); }
        __device__ __forceinline__ void set_e(uint32_t q, uint32_t v) { if (col == q) xe = v; }
        __device__ __forceinline__ void set_g(uint32_t q, uint32_t v) { if (col == q) xg = v; }
      } rows{xe, xg, col, wb, dim};
      close_tail_gaps(rows, dim, (uint32_t)(j + (int)matches + 1), est_cl, gen_cl);
      if (gen_cl >= 0 && est_cl >= 0 && est_cl < (int)n && gen_cl < (int)m) {
        sub_la = (uint32_t)est_cl + 1u; sub_lb = (uint32_t)gen_cl + 1u;
        valid = true;
      }
    }
  }
  if (!valid || sub_lb == 0u) return;                          // (an exon that is empty on the genomic sequence gets no check)
  // the exon check of the trimmed exon: a = the exon on the genomic sequence, b = on the EST (include/pintron_gpu.h)
  DevJob sub = job;
  sub.a = job.b + sub_b_off; sub.la = sub_lb;
  sub.b = job.a + sub_a_off; sub.lb = sub_la;
  sub.p0 = max_edit_for_exon(sub_lb);
  sub.tail = 1u;
  const uint32_t big = sub.la > sub.lb ? sub.la : sub.lb, sml = sub.la > sub.lb ? sub.lb : sub.la;
  if (!((2u * sub.p0 + 1u < big && 2u * sub.p0 + 1u <= 64u) || sml <= 64u)) return;      // more than one row per lane
  if (lane == 0) { tmp->status = 1; tmp->v[0] = 0; tmp->v[1] = 0; tmp->v[2] = 0; }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  lev_wave_body<1, MODE_KBAND>(sub, tmp, ws, lane);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0 && tmp->status == 0) {
    res->v[2] = (int32_t)(job.p0 == 1u ? sub_a_off : sub_la);
    res->v[3] = (int32_t)(job.p0 == 1u ? sub_b_off : sub_lb);
    res->v[4] = (int32_t)((tmp->v[0] ? 1u : 0u) | (((uint32_t)tmp->v[2] & 3u) << 1) | 8u | (sub.p0 << 8));
  }
}

// ---------------------------------------------------------------------------------------------
// ONE launch for every wave-per-job family of a batch (the wave-job role of dp_batch_kernel).  A batch used to cost eleven launches
// dealt onto four hardware queues, and the kernels of a queue run one after the other: the batch
// took the SUM of its families' long poles per queue.  Here every wave of the grid looks its job up
// in a short segment table (family, first job, count; long-running families first) and runs that
// family's body: alignments with their tracebacks, gap alignments with theirs, banded and plain edit
// distances and the single-wave BORDERS / AFFIX jobs overlap inside one dispatch, and the batch costs
// its longest job.  The rare large row classes (BIG instances, a few hundred registers per lane) and
// the one-job-per-workgroup kernels keep launches of their own.
// ---------------------------------------------------------------------------------------------
constexpr size_t WAVE_JOBS_LDS = 4 * (size_t)TB_WIN_BYTES + 4 * (size_t)TB_PATH + 4 * 4 * 65 * sizeof(uint32_t);
static_assert(WAVE_JOBS_LDS + 256 <= 40 * 1024, "four workgroups of dp_batch_kernel per CU (160 KB of LDS; 256 B are static)");

// wave `wave` (0..3) of workgroup `block` of the wave-per-job part; smem: WAVE_JOBS_LDS bytes, 16-aligned
__device__ __forceinline__ void wave_jobs_body(const int block, const int wave, const uint32_t lane,
                                               const DevJob* __restrict__ jobs, const WaveSegs& segs,
                                               DevResult* __restrict__ results, uint8_t* __restrict__ ws,
                                               uint8_t* __restrict__ strs, uint8_t* smem, const LcfIndexView& ix) {
  uint8_t* s_win = smem + (size_t)wave * TB_WIN_BYTES;
  uint8_t* s_path = smem + 4 * (size_t)TB_WIN_BYTES + (size_t)wave * TB_PATH;
  uint32_t* s_borders = reinterpret_cast<uint32_t*>(smem + 4 * (size_t)TB_WIN_BYTES + 4 * (size_t)TB_PATH) + wave * (4 * 65);
  int w = block * 4 + wave, fam = -1, idx = 0;
  for (int sgi = 0; sgi < segs.n; ++sgi) {
    if (w < segs.count[sgi]) { fam = segs.family[sgi]; idx = segs.start[sgi] + w; break; }
    w -= segs.count[sgi];
  }
  if (fam < 0) return;
  const DevJob job = jobs[idx];
  DevResult* res = &results[job.out_idx];
  switch (fam) {
    case KF_ALIGN:                       // up to 64 rows (the rest are on four waves: align_coop_body)
      lev_wave_body<1, MODE_ALIGN>(job, res, ws, lane);
      own_stores_visible();
      align_traceback_wave(job, res, ws, strs, lane, s_win, s_path);
      if (job.p0 != 0u) { own_stores_visible(); endpoint_epilogue(job, res, strs, ws, lane, reinterpret_cast<DevResult*>(s_borders)); }
      break;
    case KF_GAP:
      switch (job.r_class) {
        case 1:  gap_wave_body<1>(job, res, ws, lane); break;
        case 2:  gap_wave_body<2>(job, res, ws, lane); break;
        default: gap_wave_body<4>(job, res, ws, lane); break;
      }
      own_stores_visible();
      gap_traceback_wave(job, res, ws, strs, lane, s_win, s_path);
      break;
    case KF_KBAND:   lev_any_dispatch<MODE_KBAND, false>(job, res, ws, lane); break;
    case KF_ED:      lev_any_dispatch<MODE_ED, false>(job, res, ws, lane); break;
    case KF_BORDERS: lev_wave_body<1, MODE_BORDERS>(job, res, ws, lane, s_borders); break;
    case KF_AFFIX:   lev_wave_body<1, MODE_AFFIX>(job, res, ws, lane); break;
    case KF_LCFSA:   lcfsa_wave_body(job, res, ix, lane, reinterpret_cast<uint8_t*>(s_borders)); break;
    case KF_LCFW:    lcf_small_wave_body(job, res, lane); break;
    case KF_ALIGNB: {                    // see align_band_sweep; the host chose the jobs (more than 64 rows, lengths within the band)
      const uint32_t n = job.la, m = job.lb;
      bool same = n == m;
      if (same) for (uint32_t q = lane; q < n; q += 64) same = same && job.a[q] == job.b[q];
      if (__all(same)) {                 // identity alignment, score 0 (compute-alignments.c:48-58)
        if (lane == 0) { res->status = 0; res->v[0] = 0; res->v[1] = (int32_t)n; res->v[5] = 1; }
        own_stores_visible();
        align_traceback_wave(job, res, ws, strs, lane, s_win, s_path);      // its identity branch
        if (job.p0 != 0u) { own_stores_visible(); endpoint_epilogue(job, res, strs, ws, lane, reinterpret_cast<DevResult*>(s_borders)); }
        break;
      }
      uint32_t* bdirs = reinterpret_cast<uint32_t*>(ws + job.ws_off);
      const uint32_t score = align_band_sweep(job.a, n, job.b, m, lane, bdirs);
      if (score > ALIGN_BAND_K) { if (lane == 0) res->status = ALIGN_BAND_RETRY; break; }
      if (lane == 0) { res->status = 0; res->v[0] = (int32_t)score; res->v[5] = 0; }
      own_stores_visible();
      align_band_traceback(job, res, bdirs, strs, lane, s_win, s_path);
      if (job.p0 != 0u) { own_stores_visible(); endpoint_epilogue(job, res, strs, ws, lane, reinterpret_cast<DevResult*>(s_borders)); }
      break;
    }
    default: break;
  }
}

// follow-up of the batch launch: the banded ALIGN jobs whose score exceeded the band, on four waves each;
// a workgroup whose job is settled (nearly all) ends at once
__global__ __launch_bounds__(256)
void align_fallback_kernel(const DevJob* __restrict__ jobs, int njobs, DevResult* __restrict__ results,
                           uint8_t* __restrict__ ws, uint8_t* __restrict__ strs) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[ALIGN_COOP_LDS];
  const DevJob job = jobs[blockIdx.x];
  if (results[job.out_idx].status != ALIGN_BAND_RETRY) return;
  align_coop_dispatch(job, &results[job.out_idx], ws, strs, smem);
}

// ---------------------------------------------------------------------------------------------
// ONE launch for everything of a batch that is bound by the latency of its longest job: the
// one-job-per-workgroup sweeps (BORDERS on eight waves, AFFIX on four) and the wave-per-job
// families.  Workgroups of 512 threads; the role of a workgroup follows from its index -- the long
// poles first, so they start first: [BORDERS coop jobs][AFFIX coop jobs][wave-job groups of four].
// The roles with four waves let the upper four end at once (s_barrier only waits for the waves of
// a workgroup that have not ended).  All roles share the dynamic LDS.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512)
void dp_batch_kernel(const DevJob* __restrict__ jobs, const BatchDesc d, DevResult* __restrict__ results,
                     uint8_t* __restrict__ ws, uint8_t* __restrict__ strs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t batch_lds[];
  int b = (int)blockIdx.x;
  if (b < d.bc_count) {
    const DevJob job = jobs[d.bc_start + b];
    borders_coop_dispatch(job, &results[job.out_idx]);      // its LDS is the dynamic array
    return;
  }
  b -= d.bc_count;
  if (threadIdx.x >= 256) return;
  if (b < d.ac_count) {
    const DevJob job = jobs[d.ac_start + b];
    uint32_t* hand = reinterpret_cast<uint32_t*>(batch_lds);
    uint32_t (*wbest)[5] = reinterpret_cast<uint32_t (*)[5]>(batch_lds + (COOP_W - 1) * 128 * sizeof(uint32_t));
    affix_coop_dispatch(job, &results[job.out_idx], hand, wbest);
    return;
  }
  b -= d.ac_count;
  if (b < d.lc_count) {
    const DevJob job = jobs[d.lc_start + b];
    align_coop_dispatch(job, &results[job.out_idx], ws, strs, batch_lds);
    return;
  }
  b -= d.lc_count;
  const int wave = (int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  wave_jobs_body(b, wave, threadIdx.x & 63u, jobs, d.segs, results, ws, strs, batch_lds, d.ix);
}
constexpr size_t AFFIX_COOP_LDS = (COOP_W - 1) * 128 * sizeof(uint32_t) + COOP_W * 5 * sizeof(uint32_t);

// ---------------------------------------------------------------------------------------------
// Longest common factor with N wildcard: find_longest_common_factor_dp
// (src/factorization-refinement.c:255-316).  curr[i2+1] = match ? prev[i2]+1 : 0 only couples
// cells of one diagonal, so the l1+l2-1 diagonals are independent: one thread per diagonal,
// 256 diagonals per workgroup, a tile of s1 and the whole of s2 staged in LDS.  The reference
// keeps the FIRST maximum in (i1,i2) scan order == among maximal runs the smallest start in s1,
// then in s2; that order is folded into a 64-bit key reduced with atomicMax.
// ---------------------------------------------------------------------------------------------
constexpr int LCF_BLOCK = 256;
constexpr uint32_t LCF_MAX_L2 = 65535u;

// grid (workgroups per job, jobs); keys[job] (zeroed by the caller) collects the best key of the job's
// workgroups.  The host turns the keys into results (pgpu_dp_plan_sync): a finish pass on the device
// would cost a launch per batch, and "the last workgroup finishes" needs device-scope fences, i.e. a
// write-back and an invalidation of the XCD's L2 per workgroup -- measured: six times slower, and every
// kernel running beside it with it.
__global__ __launch_bounds__(LCF_BLOCK)
void lcf_kernel(const DevJob* __restrict__ jobs, int njobs, unsigned long long* __restrict__ keys) {
  extern __shared__ uint8_t lcf_lds[];         // [s2: l2 bytes][s1 tile: LCF_BLOCK + l2 bytes]
  __shared__ unsigned long long wbest[LCF_BLOCK / 64];
  const DevJob job = jobs[blockIdx.y];
  const uint32_t l1 = job.la, l2 = job.lb;
  unsigned long long best = 0;
  if (l1 != 0 && l2 != 0) {                    // uniform over the workgroup
    uint8_t* s2 = lcf_lds;
    uint8_t* tile = lcf_lds + ((l2 + 15u) & ~15u);
    for (uint32_t i = threadIdx.x; i < l2; i += LCF_BLOCK) s2[i] = job.b[i];
    const uint32_t ndiag = l1 + l2 - 1;
    const uint32_t nchunks = (ndiag + LCF_BLOCK - 1) / LCF_BLOCK;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
      // diagonal index dg in [0, ndiag): i1 - i2 = dg - (l2-1).  This chunk covers s1 positions
      // [base, base + LCF_BLOCK + l2 - 1) where base = chunk*LCF_BLOCK - (l2-1) (may be negative)
      const int64_t base = (int64_t)chunk * LCF_BLOCK - (int64_t)(l2 - 1);
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < LCF_BLOCK + l2 - 1; i += LCF_BLOCK) {
        const int64_t g = base + i;
        tile[i] = (g >= 0 && g < (int64_t)l1) ? job.a[g] : 0;
      }
      __syncthreads();
      const uint32_t dg = chunk * LCF_BLOCK + threadIdx.x;
      if (dg < ndiag) {
        // cells of this diagonal: i2 from max(0, l2-1-dg), i1 = i2 + dg - (l2-1)
        const uint32_t i2_lo = dg < l2 - 1 ? l2 - 1 - dg : 0;
        const int64_t shift = (int64_t)dg - (int64_t)(l2 - 1);       // i1 - i2
        uint32_t i2_hi = l2;                                          // exclusive
        if ((int64_t)l1 - shift < (int64_t)i2_hi) i2_hi = (uint32_t)((int64_t)l1 - shift);
        uint32_t run = 0, brun = 0, bend = 0;
        for (uint32_t i2 = i2_lo; i2 < i2_hi; ++i2) {
          const uint32_t c1 = tile[threadIdx.x + i2];                // s1[i2 + shift] = tile[i2+shift-base]
          const uint32_t c2 = s2[i2];
          run = (c1 == c2 || is_n(c1) || is_n(c2)) ? run + 1 : 0;
          if (run > brun) { brun = run; bend = i2; }
        }
        if (brun > 0) {
          const uint32_t occ2 = bend + 1 - brun;
          const uint32_t occ1 = (uint32_t)((int64_t)occ2 + shift);
          const unsigned long long key = lcf_key(brun, occ1, occ2);
          best = key > best ? key : best;
        }
      }
    }
    // workgroup reduction, one atomic per workgroup
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off);
      best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (l1 != 0 && l2 != 0) {
      for (int wv = 1; wv < LCF_BLOCK / 64; ++wv) best = wbest[wv] > best ? wbest[wv] : best;
      if (best) atomicMax(&keys[blockIdx.y], best);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Jobs beyond the row limits of the register-resident kernels (GAP windows of more than 2048 EST
// characters, BORDERS patterns of more than 4096): the reference computes them, slowly, so they
// must not be refused.  One workgroup per job walks the anti-diagonals of the matrix with three
// rolling diagonals per plane in the job's HBM workspace; cell (i, j) only needs diagonals d-1 and
// d-2, thread q owns the rows i = q+1, q+1+256, ...  Nothing here is tuned: such jobs are rare
// (long reads with a long unaligned stretch) and a slow answer beats an abort.
// ---------------------------------------------------------------------------------------------
constexpr int SLOW_BLOCK = 256;

// ComputeGapAlignMatrix + TracebackGapAlignment (src/refine-intron.c:623-890), semantics as in
// gap_wave_body / gap_traceback_wave.  Workspace: [9 x (n+1) int32 rolling diagonals][(n+1)*(m+1) bytes:
// bits 0-1 L direction, bit 2 G "came from L", bits 3-4 R direction (3 = came from G)]
__global__ __launch_bounds__(SLOW_BLOCK)
void gap_slow_kernel(const DevJob* __restrict__ jobs, int njobs, DevResult* __restrict__ results,
                     uint8_t* __restrict__ ws, uint8_t* __restrict__ strs) {
  const DevJob job = jobs[blockIdx.x];
  DevResult* res = &results[job.out_idx];
  const uint32_t n = job.la, m = job.lb, cap = n + m + 1;
  int32_t* diag = (int32_t*)(ws + job.ws_off);
  uint8_t* dirs = ws + job.ws_off + (size_t)9 * (n + 1) * sizeof(int32_t);
  const size_t w = (size_t)m + 1;
  auto plane = [&](int which, uint32_t d) -> int32_t* { return diag + ((size_t)(which * 3 + (int)(d % 3u))) * (n + 1); };
  for (uint32_t d = 2; d <= n + m; ++d) {
    const int32_t *L1 = plane(0, d - 1), *L2 = plane(0, d - 2), *G1 = plane(1, d - 1), *R1 = plane(2, d - 1), *R2 = plane(2, d - 2);
    int32_t *Lc = plane(0, d), *Gc = plane(1, d), *Rc = plane(2, d);
    for (uint32_t i = threadIdx.x + 1; i <= n; i += SLOW_BLOCK) {
      if (d <= i) break;
      const uint32_t j = d - i;
      if (j > m) continue;
      // neighbours on the zero border (row 0 / column 0 of every plane) read as 0
      const bool up_ok = i > 1, left_ok = j > 1;
      const uint32_t ce = job.a[i - 1], cg = job.b[j - 1];
      const int32_t sub = (ce == cg || is_n(ce) || is_n(cg)) ? 1 : -1;
      const int32_t l_diag = (up_ok && left_ok) ? L2[i - 1] : 0, l_up = up_ok ? L1[i - 1] : 0, l_left = left_ok ? L1[i] : 0;
      const int32_t g_left = left_ok ? G1[i] : 0;
      const int32_t r_diag = (up_ok && left_ok) ? R2[i - 1] : 0, r_up = up_ok ? R1[i - 1] : 0, r_left = left_ok ? R1[i] : 0;
      int32_t v = l_diag + sub; uint32_t dl = 0;
      if (v < l_up - 1) { v = l_up - 1; dl = 1; }
      if (v < l_left - 1) { v = l_left - 1; dl = 2; }
      Lc[i] = v;
      v = g_left; uint32_t dg = 0;
      if (v < l_left) { v = l_left; dg = 1; }
      Gc[i] = v;
      v = r_diag + sub; uint32_t dr = 0;
      const int32_t left = (i != n) ? r_left - 1 : r_left;            // free trailing gap (:756-759)
      if (v < left) { v = left; dr = 2; }
      if (v < g_left) { v = g_left; dr = 3; }
      if (v < r_up - 1) { v = r_up - 1; dr = 1; }
      Rc[i] = v;
      dirs[(size_t)i * w + j] = (uint8_t)(dl | (dg << 2) | (dr << 3));
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  uint8_t* ea = strs + job.str_off;
  uint8_t* ga = ea + cap;
  int32_t pl = 0;
  if (n > 0 && m > 0) {
    const uint32_t d = n + m;
    const int32_t l = plane(0, d)[n], g = plane(1, d)[n], r = plane(2, d)[n];
    if (r >= g) pl = (r >= l) ? 2 : 0; else pl = (g >= l) ? 1 : 0;   // :808-819
  } else pl = 2;                                                   // all three are 0
  int32_t factor_cut = 0, intron_start = 0, intron_end = 0, rev_start = -1, rev_end = -1;
  uint32_t i = n, j = m, pos = cap - 1, k = 0;
  ea[pos] = 0; ga[pos] = 0;
  while (i > 0 && j > 0) {
    const uint32_t b = dirs[(size_t)i * w + j];
    const uint32_t dd = pl == 2 ? ((b >> 3) & 3u) : (pl == 1 ? (((b >> 2) & 1u) ? 3u : 2u) : (b & 3u));
    --pos;
    if (dd == 0)      { ea[pos] = job.a[--i]; ga[pos] = job.b[--j]; }
    else if (dd == 1) { ea[pos] = job.a[--i]; ga[pos] = '-'; }
    else {
      if (dd == 3) {
        if (pl == 2) { intron_end = (int32_t)j - 1; factor_cut = (int32_t)i; rev_end = (int32_t)k; }
        else         { intron_start = (int32_t)j - 1; rev_start = (int32_t)k; }
        --pl;
      }
      ea[pos] = '-'; ga[pos] = job.b[--j];
    }
    ++k;
  }
  while (i > 0) { --pos; ea[pos] = job.a[--i]; ga[pos] = '-'; ++k; }
  while (j > 0) { --pos; ea[pos] = '-'; ga[pos] = job.b[--j]; ++k; }
  res->status = 0;
  res->v[0] = (int32_t)k; res->v[1] = factor_cut; res->v[2] = intron_start; res->v[3] = intron_end;
  res->v[4] = rev_start >= 0 ? (int32_t)k - 1 - rev_start : 0;
  res->v[5] = rev_end >= 0 ? (int32_t)k - 1 - rev_end : 0;
  res->pad = 0;
  res->str[0] = job.str_off + pos;
  res->str[1] = job.str_off + cap + pos;
}

// general_refine_borders (src/refine.c:105-192) for patterns of more than 4096 characters.
// Workspace: [3 x (len_p+1) uint32 rolling diagonals][pre, pre_pos, suf, suf_pos: 4 x (len_p+1) uint32]
__global__ __launch_bounds__(SLOW_BLOCK)
void borders_slow_kernel(const DevJob* __restrict__ jobs, int njobs, DevResult* __restrict__ results, uint8_t* __restrict__ ws) {
  const DevJob job = jobs[blockIdx.x];
  DevResult* res = &results[job.out_idx];
  const uint32_t len_p = job.la, len_t = job.lb, max_errs = job.p2;
  const uint32_t t_win = min(len_p + max_errs, len_t);
  uint32_t* diag = (uint32_t*)(ws + job.ws_off);
  const BordersMins mins{diag + (size_t)3 * (len_p + 1), len_p};
  for (int sweep = 0; sweep < 2; ++sweep) {
    uint32_t* mv = sweep ? mins.suf : mins.pre;
    uint32_t* mp = sweep ? mins.suf_pos : mins.pre_pos;
    const Operand rows{job.a, len_p, sweep == 1}, cols{job.b, len_t, sweep == 1};
    for (uint32_t i = threadIdx.x; i <= len_p; i += SLOW_BLOCK) { mv[i] = i; mp[i] = 0; }     // column 0: M[i][0] = i
    __syncthreads();
    for (uint32_t d = 2; d <= len_p + t_win; ++d) {
      const uint32_t *D1 = diag + (size_t)((d - 1) % 3u) * (len_p + 1), *D2 = diag + (size_t)((d - 2) % 3u) * (len_p + 1);
      uint32_t* Dc = diag + (size_t)(d % 3u) * (len_p + 1);
      for (uint32_t i = threadIdx.x + 1; i <= len_p; i += SLOW_BLOCK) {
        if (d <= i) break;
        const uint32_t j = d - i;
        if (j > t_win) continue;
        const uint32_t dg = i == 1 ? j - 1 : (j == 1 ? i - 1 : D2[i - 1]);
        const uint32_t up = i == 1 ? j : D1[i - 1];
        const uint32_t lf = j == 1 ? i : D1[i];
        uint32_t v = dg + (rows.at(i - 1) == cols.at(j - 1) ? 0u : 1u);
        if (v > up + 1) v = up + 1;
        if (v > lf + 1) v = lf + 1;
        Dc[i] = v;
        if (mv[i] > v) { mv[i] = v; mp[i] = j; }            // strict: the first arg-min of the row (:133-159)
      }
      __syncthreads();
    }
  }
  if (threadIdx.x != 0) return;
  // the scan of src/refine.c:161-178 as the reference writes it, by thread 0
  const uint32_t *pre = mins.pre, *pre_pos = mins.pre_pos, *suf = mins.suf, *suf_pos = mins.suf_pos;
  const uint32_t avail = len_t + min(job.tail, 2u);
  const uint32_t lo = job.p0, hi = job.p1 > job.p0 ? job.p1 : job.p0;
  uint32_t bi = lo, bc = pre[lo] + suf[len_p - lo];
  int bf = burset_adaptor(job.b, avail, pre_pos[lo], len_t - suf_pos[len_p - lo]);
  for (uint32_t i = lo + 1; i <= hi; ++i) {
    const int freq = burset_adaptor(job.b, avail, pre_pos[i], len_t - suf_pos[len_p - i]);
    const uint32_t c = pre[i] + suf[len_p - i];
    if (bc > c || (bc == c && freq > bf)) { bc = c; bf = freq; bi = i; }
  }
  borders_write_result(job, res, pre_pos, suf_pos, bi, bc);
}

}  // namespace

// What dp_batch_kernel leaves to launches of their own (one launcher per stand-alone route of the plan builder's
// table; a group that is launched is never empty).  ED, ALIGN, KBAND: the large row classes, all of them BIG
// instances (see lev_any_dispatch).
template <int MODE>
static void launch_lev_any(const DpLaunch& l) {
  hipLaunchKernelGGL(lev_any_kernel<MODE>, dim3((l.njobs + 3) / 4), dim3(256), 0, l.st, l.jobs, l.njobs, l.res, l.ws, l.strs);
}
void launch_ed_big(const DpLaunch& l) { launch_lev_any<MODE_ED>(l); }
void launch_align_big(const DpLaunch& l) { launch_lev_any<MODE_ALIGN>(l); }
void launch_kband_big(const DpLaunch& l) { launch_lev_any<MODE_KBAND>(l); }

void launch_borders_slow(const DpLaunch& l) {
  hipLaunchKernelGGL(borders_slow_kernel, dim3(l.njobs), dim3(SLOW_BLOCK), 0, l.st, l.jobs, l.njobs, l.res, l.ws);
}

void launch_borders_coop(const DpLaunch& l) {
  const size_t lds = (2 * (COOP_W - 1) * 128 + 4 * ((size_t)l.max_rows + 1)) * sizeof(uint32_t);
  hipLaunchKernelGGL(borders_coop_any_kernel, dim3(l.njobs), dim3(512), lds, l.st, l.jobs, l.njobs, l.res);
}

void launch_affix_strips(const DpLaunch& l) {
  hipLaunchKernelGGL((lev_wave_kernel<64, MODE_AFFIX, true>), dim3((l.njobs + 3) / 4), dim3(256), 0, l.st, l.jobs, l.njobs, l.res, l.ws);
}

void launch_align_fallback(const DevJob* jobs, int njobs, DevResult* res, uint8_t* ws, uint8_t* strs, hipStream_t st) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(align_fallback_kernel, dim3(njobs), dim3(256), 0, st, jobs, njobs, res, ws, strs);
}

void launch_gap_slow(const DpLaunch& l) {
  hipLaunchKernelGGL(gap_slow_kernel, dim3(l.njobs), dim3(SLOW_BLOCK), 0, l.st, l.jobs, l.njobs, l.res, l.ws, l.strs);
}

void launch_gap_big(const DpLaunch& l) {
  hipLaunchKernelGGL(gap_any_kernel, dim3((l.njobs + 3) / 4), dim3(256), 0, l.st, l.jobs, l.njobs, l.res, l.ws, l.strs);
}

void launch_lcf(const DpLaunch& l) {
  // grid.y = job (<= 65535 per launch, the caller slices), grid.x strides over diagonal chunks
  // ... as many workgroups per job as it takes to fill the chip: after the suffix-array path took the ordinary
  // jobs, what comes here is a handful of long ones (an N in the EST prefix) -- 64 workgroups each left three
  // quarters of the CUs idle and made these launches the long pole of their batches
  uint32_t want = 4096u / (uint32_t)l.njobs;
  if (want < 64u) want = 64u;
  const uint32_t gx = l.max_chunks < want ? (l.max_chunks ? l.max_chunks : 1u) : want;
  // LDS: s2 (rounded to 16) + s1 tile (256 + l2 - 1), sized for the largest l2 of the launch
  const size_t lds = ((l.max_l2 + 15u) & ~15u) + LCF_BLOCK + l.max_l2;
  hipLaunchKernelGGL(lcf_kernel, dim3(gx, l.njobs), dim3(LCF_BLOCK), lds, l.st, l.jobs, l.njobs, l.keys);
}

size_t dp_batch_lds_bytes(bool wave_jobs, int bc_count, uint32_t bc_max_rows, int ac_count, int lc_count) {
  size_t lds = 16;
  if (wave_jobs) lds = std::max(lds, WAVE_JOBS_LDS);
  if (ac_count > 0) lds = std::max(lds, AFFIX_COOP_LDS);
  if (lc_count > 0) lds = std::max(lds, ALIGN_COOP_LDS);
  if (bc_count > 0) lds = std::max(lds, (2 * (COOP_W - 1) * 128 + 4 * ((size_t)bc_max_rows + 1)) * sizeof(uint32_t));
  return lds;
}

bool launch_dp_batch(const DevJob* jobs, const BatchDesc& d, uint32_t bc_max_rows, DevResult* res, uint8_t* ws, uint8_t* strs,
                     hipStream_t st) {
  const int blocks = d.bc_count + d.ac_count + d.lc_count + d.wave_blocks;
  if (blocks == 0) return true;
  const size_t lds = dp_batch_lds_bytes(d.wave_blocks > 0, d.bc_count, bc_max_rows, d.ac_count, d.lc_count);
  if (lds > DP_BATCH_MAX_LDS) return false;
  hipLaunchKernelGGL(dp_batch_kernel, dim3(blocks), dim3(512), lds, st, jobs, d, res, ws, strs);
  return true;
}
