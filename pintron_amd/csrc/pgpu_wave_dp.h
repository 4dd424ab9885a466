// The wave-per-job pieces of the dynamic programs that more than one translation unit runs: the DPP wave shifts, the
// traceback's LDS window and write-out, and the 3-state gap alignment (sweep and traceback).  pgpu_dp_kernels.hip runs
// them as PGPU_DP_GAP jobs of a plan, pgpu_chain.hip as one step of a chain of introns.  The scheme (row strips x skewed
// column sweep, step-major direction bytes, scalar walk in an LDS window) is described at the top of pgpu_dp_kernels.hip.
#pragma once

#include "pgpu_internal.h"

namespace {

constexpr uint32_t PAD_ROW = 0x01u;   // never equal to a sequence byte nor to PAD_COL
constexpr uint32_t PAD_COL = 0x02u;

__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
  // DPP wave_shr:1 -- lane l receives lane l-1's v; lane 0 keeps its own (overwritten by caller)
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ uint32_t wave_shl1(uint32_t v) {
  // DPP wave_shl:1 -- lane l receives lane l+1's v; lane 63 keeps its own (the caller masks it)
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xf, 0xf, false);
}
// lane l receives lane l-1's v, lane 0 receives ITS OWN `first` (a lane without a source keeps the old value)
__device__ __forceinline__ uint32_t wave_shr1_first(uint32_t first, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)v, 0x138, 0xf, 0xf, false);
}
// lane l receives lane l+1's v, lane 63 receives its own `last`
__device__ __forceinline__ uint32_t wave_shl1_last(uint32_t last, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)last, (int)v, 0x130, 0xf, 0xf, false);
}

__device__ __forceinline__ bool is_n(uint32_t c) { return c == 'n' || c == 'N'; }

constexpr int TB_WIN_BYTES = 8192;    // traceback: direction window per wave
// traceback: path steps buffered before the lanes write them out.  704, not 1024: with it a workgroup of dp_batch_kernel
// takes 39 744 + 256 B of LDS, and FOUR of them share a CU's 160 KB (16 job waves, what the registers allow) instead of three
constexpr int TB_PATH = 704;

// The wave that filled a traceback workspace walks it right away (ALIGN, GAP): what it stored has
// to be visible to its other lanes, and lines of an earlier batch may sit in this CU's L1.
__device__ __forceinline__ void own_stores_visible() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// the write-out of a traceback (align_traceback_wave, gap_traceback_wave): the gapped strings of the path steps buffered so far
__device__ __forceinline__ void tb_flush(const uint8_t* path, uint32_t np, const uint8_t* a, const uint8_t* b,
                                         uint32_t i0, uint32_t j0, uint32_t pos0, uint8_t* ea, uint8_t* ga,
                                         uint32_t lane) {
  uint32_t ca = 0, cb = 0;             // characters of a / b consumed by the steps before this group
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (uint32_t base = 0; base < np; base += 64) {
    const uint32_t idx = base + lane;
    const bool valid = idx < np;
    const uint32_t d = valid ? path[idx] : 1u;
    const bool ua = valid && d <= 1u, ub = valid && d != 1u;       // step consumes a[..] / b[..] (2, 3: b only)
    const unsigned long long ma = __ballot(ua), mb = __ballot(ub);
    if (valid) {
      const uint32_t ia = i0 - 1u - (ca + (uint32_t)__popcll(ma & lt));
      const uint32_t ib = j0 - 1u - (cb + (uint32_t)__popcll(mb & lt));
      ea[pos0 - 1u - idx] = ua ? a[ia] : (uint8_t)'-';
      ga[pos0 - 1u - idx] = ub ? b[ib] : (uint8_t)'-';
    }
    ca += (uint32_t)__popcll(ma); cb += (uint32_t)__popcll(mb);
  }
}

// ---------------------------------------------------------------------------------------------
// 3-state gap alignment: ComputeGapAlignMatrix with only_one_align (src/refine-intron.c:623-824)
// ---------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void gap_wave_body(const DevJob& job, DevResult* res, uint8_t* __restrict__ ws,
                                              const uint32_t lane) {
  const uint32_t n = job.la, m = job.lb;
  int32_t cL[R], cG[R], cR[R];
  uint32_t rc[R];
  const uint32_t row0 = lane * R;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    rc[r] = row0 + r < n ? job.a[row0 + r] : PAD_ROW;
    cL[r] = 0; cG[r] = 0; cR[r] = 0;                       // column 0 of every plane is 0
  }
  if (n > 0 && m > 0) {
    const uint32_t last_lane = (n - 1) / R, steps = m + last_lane;
    int32_t dgL = 0, dgR = 0;                               // row above the strip, previous column
    uint32_t out = 0, outc = 0;
    uint8_t* dirs = ws + job.ws_off;
    // per 64-step chunk the column characters sit in `feed` (lane t = step t), which moves one lane
    // down per step: lane 0 always holds the current one (see lev_sweep)
    uint32_t feed_next = lane < m ? job.b[lane] : PAD_COL;        // requested one chunk ahead (see lev_sweep)
    for (uint32_t s0 = 0; s0 < steps; s0 += 64) {
      uint32_t feed = feed_next;
      const uint32_t jn = s0 + 64u + lane;
      feed_next = jn < m ? job.b[jn] : PAD_COL;
      const uint32_t tmax = (min(64u, steps - s0) + 7u) & ~7u;   // whole groups of 8; steps past the end touch no cell
      for (uint32_t t0 = 0; t0 < tmax; t0 += 8) {
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
          const uint32_t s = s0 + t0 + u;
          const uint32_t in = wave_shr1_first(0u, out);         // row 0 of L and R is 0
          const uint32_t inc = wave_shr1_first(feed, outc);
          feed = wave_shl1(feed);
          const uint32_t j = s - lane + 1;
          if (j - 1u < m) {
            const uint32_t ch = inc;
            const int32_t inL = (int32_t)(int16_t)(in & 0xFFFFu), inR = (int32_t)(int16_t)(in >> 16);
            int32_t upL = inL, upR = inR, diagL = dgL, diagR = dgR;
            const bool ch_n = is_n(ch);
            uint32_t packed[(R + 3) / 4];
#pragma unroll
            for (int q = 0; q < (R + 3) / 4; ++q) packed[q] = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const int32_t leftL = cL[r], leftG = cG[r], leftR = cR[r];
              const int32_t sub = (rc[r] == ch || ch_n || is_n(rc[r])) ? 1 : -1;
              // L plane: diag, up (1), left (2); strict '<' replaces
              int32_t v = diagL + sub; uint32_t dl = 0;
              if (v < upL - 1) { v = upL - 1; dl = 1; }
              if (v < leftL - 1) { v = leftL - 1; dl = 2; }
              // G plane: stay (2) or enter from L (-2)
              int32_t g = leftG; uint32_t dg = 0;
              if (g < leftL) { g = leftL; dg = 1; }
              // R plane: diag, left (2; free in the last EST row), from G (-2), up (1)
              int32_t rv = diagR + sub; uint32_t dr = 0;
              const int32_t lc = (row0 + r + 1 != n) ? leftR - 1 : leftR;
              if (rv < lc) { rv = lc; dr = 2; }
              if (rv < leftG) { rv = leftG; dr = 3; }
              if (rv < upR - 1) { rv = upR - 1; dr = 1; }
              packed[r / 4] |= (dl | (dg << 2) | (dr << 3)) << (8 * (r % 4));
              diagL = leftL; diagR = leftR;
              cL[r] = v; cG[r] = g; cR[r] = rv;
              upL = v; upR = rv;
            }
            dgL = inL; dgR = inR;
            out = ((uint32_t)upL & 0xFFFFu) | ((uint32_t)upR << 16);
            outc = ch;
            uint8_t* p = dirs + ((size_t)s * 64 + lane) * R;
            if constexpr (R == 1)      *p = (uint8_t)packed[0];
            else if constexpr (R == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)packed[0];
            else if constexpr (R == 4) *reinterpret_cast<uint32_t*>(p) = packed[0];
            else if constexpr (R == 8) *reinterpret_cast<uint2*>(p) = make_uint2(packed[0], packed[1]);
            else {
#pragma unroll
              for (int q = 0; q < R / 16; ++q)
                reinterpret_cast<uint4*>(p)[q] =
                    make_uint4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]);
            }
          }
        }
      }
    }
  }
  // start plane (src/refine-intron.c:808-819); with n==0 or m==0 every plane is 0 -> R
  if (n == 0 || m == 0) {
    if (lane == 0) { res->status = 0; res->pad = 2; }
    return;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (row0 + r + 1 == n) {
      const int32_t fl = cL[r], fg = cG[r], fr = cR[r];
      int plane;
      if (fr >= fg) plane = fr >= fl ? 2 : 0; else plane = fg >= fl ? 1 : 0;
      res->status = 0;
      res->pad = plane;
    }
  }
}

// TracebackGapAlignment (src/refine-intron.c:828-890), one wave per job: same scheme as
// align_traceback_wave_kernel (direction window in LDS, scalar walk, parallel write-out); the walk
// additionally carries the plane (R exon -> G intron -> L exon) and notes where it jumps.
__device__ __forceinline__ void gap_traceback_wave(const DevJob& job, DevResult* res, const uint8_t* __restrict__ ws,
                                                   uint8_t* __restrict__ strs, const uint32_t lane,
                                                   uint8_t* win, uint8_t* path) {
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.la), m = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.lb), cap = n + m + 1,
                 R = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.r_class);       // uniform walk state: see align_traceback_wave
  const uint32_t lgR = 31u - (uint32_t)__builtin_clz(R);
  const uint32_t WS = TB_WIN_BYTES / (64u * R);            // 1 B per cell: an entry is R bytes
  uint8_t* ea = strs + job.str_off;
  uint8_t* ga = ea + cap;
  const uint8_t* dirs = ws + job.ws_off;
  int plane = __builtin_amdgcn_readfirstlane(res->pad);
  int32_t factor_cut = 0, intron_start = 0, intron_end = 0;
  int32_t rev_end = -1, rev_start = -1;
  uint32_t i = n, j = m, k = 0, np = 0;
  uint32_t i0 = n, j0 = m, pos = cap - 1;
  if (lane == 0) { ea[pos] = 0; ga[pos] = 0; }
  uint32_t s_lo = 1u, s_hi = 0u;
  while (i > 0 && j > 0) {
    const uint32_t l = (i - 1) >> lgR, r = (i - 1) & (R - 1), s = (j - 1) + l;
    if (s < s_lo || s > s_hi) {
      s_hi = s; s_lo = s + 1 >= WS ? s + 1 - WS : 0;
      const uint32_t bytes = (s_hi - s_lo + 1) * 64u * R;
      const uint8_t* src = dirs + (size_t)s_lo * 64u * R;
      for (uint32_t off = lane * 16u; off < bytes; off += 64u * 16u)
        *reinterpret_cast<uint4*>(win + off) = *reinterpret_cast<const uint4*>(src + off);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    uint32_t b = win[((s - s_lo) * 64u + l) * R + r];
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    // decode to the reference's direction values: 0, 1, 2, or -2 (here 3); selects, not branches
    const uint32_t dR = (b >> 3) & 3u, dG = 2u + ((b >> 2) & 1u), dL = b & 3u;
    const uint32_t d = plane == 2 ? dR : (plane == 1 ? dG : dL);
    path[np] = (uint8_t)d;                                 // every lane, same address, same value
    const uint32_t kk = k + np;                            // steps taken before this one
    ++np;
    if (d == 3) {                                          // twice per job: the walk changes plane
      if (plane == 2) { intron_end = (int32_t)j - 1; factor_cut = (int32_t)i; rev_end = (int32_t)kk; }
      else            { intron_start = (int32_t)j - 1; rev_start = (int32_t)kk; }
      --plane;
    }
    i -= d < 2u ? 1u : 0u;
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
    res->v[0] = (int32_t)k;
    res->v[1] = factor_cut; res->v[2] = intron_start; res->v[3] = intron_end;
    res->v[4] = rev_start >= 0 ? (int32_t)k - 1 - rev_start : 0;
    res->v[5] = rev_end >= 0 ? (int32_t)k - 1 - rev_end : 0;
    res->pad = 0;
    res->str[0] = job.str_off + pos;
    res->str[1] = job.str_off + cap + pos;
  }
}

}  // namespace
