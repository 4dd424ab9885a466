// The wave-per-job pieces of the dynamic programs that more than one translation unit runs: the DPP wave shifts, the
// traceback's LDS window and write-out, and the 3-state gap alignment (sweep and traceback).  pgpu_dp_kernels.hip runs
// them as PGPU_DP_GAP jobs of a plan, pgpu_chain.hip as one step of a chain of introns.  The scheme (row strips x skewed
// column sweep, step-major direction bytes, scalar walk in an LDS window) is described at the top of pgpu_dp_kernels.hip.
// Behind the gap alignment: the Levenshtein family on one wave (lev_sweep, lev_wave_body with its modes, the dust score and
// the K-band on the lanes), the alignment's traceback, the banded alignment with its traceback, and the trimming walks of
// handle_endpoints.  pgpu_dp_kernels.hip runs them as the jobs of a plan, pgpu_clean.hip as the steps of a candidate's
// cleaning chain.
// Once, here: lev_cell, the recurrence of lev_sweep_strip and lev_sweep_coop (lev_sweep keeps its own copy: see lev_cell);
// borders_cut_scan for the wave and cooperative forms of BORDERS, BordersMins and borders_write_result for all three.
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

__device__ __forceinline__ int acgt_code(uint32_t c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -1;
  }
}

// getBursetFrequency_adaptor (src/refine-intron.c:362-374): only the BORDERS mode of lev_wave_body asks it, and a unit
// that instantiates that mode (pgpu_dp_kernels.hip, pgpu_gaps.hip) includes pgpu_burset.h, which defines it with its table
__device__ int burset_adaptor(const uint8_t* t, uint32_t avail, uint32_t cut1, uint32_t cut2);

// general_refine_borders (src/refine.c:105-192), what its wave, cooperative and slow forms share.  The row minima of the
// prefix sweep and of the reversed-string sweep with the columns where they were first reached, [pre | pre_pos | suf |
// suf_pos], each len_p + 1 words (row 0 included), carved out of one base pointer: BordersMins mins{base, len_p}.  An
// aggregate, and helpers that take the pointers by value, on purpose: a constructor, or a helper that takes the struct or
// a lane's minv[] / minpos[] by reference, changes the code the compiler makes for the sweeps beside it.
struct BordersMins {
  uint32_t* pre; uint32_t len_p;
  uint32_t* pre_pos = pre + (len_p + 1);
  uint32_t* suf = pre_pos + (len_p + 1);
  uint32_t* suf_pos = suf + (len_p + 1);
};

// the answer for the cut at pattern position bi with bc errors in all (one thread writes it)
__device__ __forceinline__ void borders_write_result(const DevJob& job, DevResult* res, const uint32_t* pre_pos,
                                                     const uint32_t* suf_pos, const uint32_t bi, const uint32_t bc) {
  const uint32_t len_p = job.la, len_t = job.lb, max_errs = job.p2;
  const uint32_t off_t1 = pre_pos[bi], off_t2 = suf_pos[len_p - bi];
  res->status = 0;
  res->v[0] = bc <= max_errs ? 1 : 0;
  res->v[1] = (int32_t)bi; res->v[2] = (int32_t)off_t1;
  res->v[3] = (int32_t)(len_t - off_t2); res->v[4] = (int32_t)bc;
}

// cut scan of src/refine.c:161-178 by one wave: the first i in [lo, hi] with the smallest total, ties by the
// larger Burset frequency.  The lanes take i = lo + lane, lo + lane + 64, ... (each reads its four
// genomic characters at once instead of lane 0 walking <= len_p+1 dependent loads) and then agree.
__device__ __forceinline__ void borders_cut_scan(const DevJob& job, DevResult* res, const uint32_t lane,
                                                 const uint32_t* pre, const uint32_t* pre_pos,
                                                 const uint32_t* suf, const uint32_t* suf_pos) {
  const uint32_t len_p = job.la, len_t = job.lb;
  const uint32_t avail = len_t + min(job.tail, 2u);
  const uint32_t lo = job.p0, hi = job.p1 > job.p0 ? job.p1 : job.p0;   // i = lo is always a candidate
  uint32_t bi = 0xFFFFFFFFu, bc = 0xFFFFFFFFu; int bf = -1;
  for (uint32_t i = lo + lane; i <= hi; i += 64) {
    const int freq = burset_adaptor(job.b, avail, pre_pos[i], len_t - suf_pos[len_p - i]);
    const uint32_t c = pre[i] + suf[len_p - i];
    if (bc > c || (bc == c && freq > bf)) { bc = c; bf = freq; bi = i; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t oc = __shfl_xor(bc, off), oi = __shfl_xor(bi, off);
    const int of = __shfl_xor(bf, off);
    if (oc < bc || (oc == bc && (of > bf || (of == bf && oi < bi)))) { bc = oc; bf = of; bi = oi; }
  }
  if (lane == 0) borders_write_result(job, res, pre_pos, suf_pos, bi, bc);
}

// ---------------------------------------------------------------------------------------------
// Levenshtein family
// ---------------------------------------------------------------------------------------------

struct Operand {            // a string read forwards or backwards
  const uint8_t* base;
  uint32_t total;           // length of the underlying buffer (for reversed reads)
  bool rev;
  __device__ __forceinline__ uint32_t at(uint32_t i) const {
    return rev ? base[total - 1 - i] : base[i];
  }
};

template <int R> struct DirPack {          // 2 bits per row, R rows
  static constexpr int WORDS = (R + 15) / 16;
  uint32_t w[WORDS];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) w[i] = 0;
  }
  __device__ __forceinline__ void set(int r, uint32_t d) { w[r / 16] |= d << (2 * (r % 16)); }
  __device__ __forceinline__ void store(uint8_t* p) const {
    if constexpr (R <= 4)       *p = (uint8_t)w[0];
    else if constexpr (R == 8)  *reinterpret_cast<uint16_t*>(p) = (uint16_t)w[0];
    else if constexpr (R == 16) *reinterpret_cast<uint32_t*>(p) = w[0];
    else if constexpr (R == 32) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    else                        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

struct AffixBest {          // running best cut of find_longest_affix; s == 0: none yet
  uint32_t v, s;            // its distance and e + g
  uint64_t key;             // (e << 32) | g: the cell scanned later has the larger key
  __device__ __forceinline__ uint32_t valid() const { return s != 0u ? 1u : 0u; }
  __device__ __forceinline__ uint32_t e() const { return (uint32_t)(key >> 32); }
  __device__ __forceinline__ uint32_t g() const { return (uint32_t)key; }
  // One cell of the scan: the cell is a candidate when the characters match and
  // 200*v <= 17*(e+g); it replaces the running best when its weight v/(e+g) is smaller, or equal
  // with a later (e,g).  `small`: e+g < 2^15, so every product fits 24x24 -> 32 bits (full-rate
  // v_mul_u32_u24); otherwise 64-bit products.  With no best yet (v = 1, s = 0) the first
  // candidate wins: cv * 0 < 1 * cs.
  template <bool SMALL>
  __device__ __forceinline__ void consider(bool match, uint32_t cv, uint32_t ce, uint32_t cg) {
    const uint32_t cs = ce + cg;
    bool cand, less, equal;
    if constexpr (SMALL) cand = match & (__umul24(200u, cv) <= __umul24(17u, cs));
    else                 cand = match & (200ull * cv <= 17ull * cs);
    // one scalar branch skips the comparison against the running best when no lane holds a candidate
    if (!__builtin_amdgcn_ballot_w64(cand)) return;
    if constexpr (SMALL) {
      const uint32_t lhs = __umul24(cv, s), rhs = __umul24(v, cs);
      less = lhs < rhs; equal = lhs == rhs;
    } else {
      const uint64_t lhs = (uint64_t)cv * s, rhs = (uint64_t)v * cs;
      less = lhs < rhs; equal = lhs == rhs;
    }
    const uint64_t ck = ((uint64_t)ce << 32) | cg;
    const bool take = cand & (less | (equal & (ck > key)));
    v = take ? cv : v; s = take ? cs : s; key = take ? ck : key;
  }
  // true when candidate o replaces this one under the reference's scan rule: smaller weight wins,
  // equal weight -> the cell scanned later (larger (e,g)) wins.
  __device__ __forceinline__ bool worse_than(const AffixBest& o) const {
    if (!s) return true;
    const uint64_t lhs = (uint64_t)o.v * s, rhs = (uint64_t)v * o.s;
    if (lhs != rhs) return lhs < rhs;
    return o.key > key;
  }
  __device__ __forceinline__ AffixBest from_lane_xor(int off) const {
    AffixBest o;
    o.v = __shfl_xor(v, off); o.s = __shfl_xor(s, off);
    o.key = ((uint64_t)__shfl_xor((uint32_t)(key >> 32), off) << 32) | __shfl_xor((uint32_t)key, off);
    return o;
  }
};
constexpr AffixBest AFFIX_NONE{1u, 0u, 0ull};

constexpr uint32_t BAND_INF = 0x3FFFFFu;   // "outside the band"; stays below the 24-bit value field

// The recurrence, once for lev_sweep_strip and lev_sweep_coop (pgpu_dp_kernels.hip): cell (row, j), the r-th of its lane.
// In: diag = M[row-1][j-1], up = M[row-1][j], cur = M[row][j-1], rcr / ch = the row's and the column's character.  Out:
// cur = up = M[row][j] and diag = M[row][j-1], i.e. what the lane's next row takes; with DIRS the cell's direction in dp,
// with ROWMIN the row's first minimum, with AFFIX the running best cut.  lev_sweep keeps the same lines written out: with
// any helper there, per column or per cell, dp_batch_kernel or lev_any_kernel<ED> fails what DESIGN.md section 8 holds them to.
template <int R, bool WILD, bool DIRS, bool ROWMIN, bool AFFIX, bool BAND, bool ASMALL>
__device__ __forceinline__ void lev_cell(const int r, const uint32_t rcr, const uint32_t ch, const bool ch_n, uint32_t& diag,
                                         uint32_t& up, uint32_t& cur, uint32_t& minv, uint32_t& minpos, AffixBest& best, DirPack<R>& dp,
                                         const uint32_t row, const uint32_t j, const uint32_t band_k) {
  const uint32_t left = cur;
  bool match = rcr == ch;
  if constexpr (WILD) match = match || ch_n || is_n(rcr);
  uint32_t v = diag + (match ? 0u : 1u);
  if constexpr (DIRS) {
    // ComputeAlignMatrix tie-break: diagonal, then up (dir 1), then left (dir 2), strict >
    uint32_t d = 0;
    if (v > up + 1) { v = up + 1; d = 1; }
    if (v > left + 1) { v = left + 1; d = 2; }
    dp.set(r, d);
  } else {
    v = min(v, min(up + 1, left + 1));
  }
  if constexpr (BAND) {
    // K_band_edit_distance keeps cells with |column - row| <= k only; neighbours outside
    // the band do not take part in the minimum (src/compute-alignments.c:375-443)
    v = (j + band_k >= row && row + band_k >= j) ? min(v, BAND_INF) : BAND_INF;
  }
  if constexpr (ROWMIN) { if (minv > v) { minv = v; minpos = j; } }   // strict: first arg-min
  // cut_weight = 2*v/(e+g) <= 0.17  <=>  200*v <= 17*(e+g)   (exact)
  if constexpr (AFFIX) best.template consider<ASMALL>(rcr == ch, v, row, j);
  diag = left; cur = v; up = v;
}

// Rows beyond 64*R are processed in horizontal STRIPS of 64*R rows by the same wave: the strip's
// last row is written, per column, to a boundary array in the job's workspace (`bottom`) and is
// the row above the first row (`top`) of the next strip; `row_base` = rows before this strip.
// The boundary values go through memory written and read by one wave: agent-scope atomics keep
// the per-CU L1 out of the way.
template <int R, bool WILD, bool DIRS, bool ROWMIN, bool AFFIX, bool BAND = false, bool ASMALL = false>
__device__ __forceinline__ void lev_sweep_strip(const Operand rows, const uint32_t nr,
                                          const Operand cols, const uint32_t nc,
                                          const uint32_t lane, uint32_t (&cur)[R],
                                          uint32_t (&minv)[R], uint32_t (&minpos)[R],
                                          AffixBest& best, uint8_t* dir_ws, const uint32_t band_k = 0,
                                          const uint32_t row_base = 0, const uint32_t* top_row = nullptr,
                                          uint32_t* bottom_row = nullptr) {
  uint32_t rc[R];                       // row characters of this lane's strip
  const uint32_t row0 = lane * R;       // rows row0+1 .. row0+R (of the strip)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = row0 + r;
    rc[r] = i < nr ? rows.at(i) : PAD_ROW;
    cur[r] = row_base + i + 1;          // M[i+1][0]
    if constexpr (BAND) { if (row_base + i + 1 > band_k) cur[r] = BAND_INF; }
    if constexpr (ROWMIN) { minv[r] = i + 1; minpos[r] = 0; }
  }
  if (nr == 0 || nc == 0) return;
  const uint32_t last_lane = (nr - 1) / R;
  const uint32_t last_r = (nr - 1) % R;
  const uint32_t steps = nc + last_lane;
  uint32_t diag_in = row_base + row0;   // M[row0][j-1] for j = 1
  uint32_t out = 0;                     // (value of the strip's last row) | (column char << 24)
  uint32_t chunk = 0, tchunk = 0;
  constexpr uint32_t EB = R <= 4 ? 1u : R / 4;
  if (bottom_row && lane == 0) {
    uint32_t b0 = row_base + nr;
    if constexpr (BAND) { if (b0 > band_k) b0 = BAND_INF; }
    __hip_atomic_store(&bottom_row[0], b0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (top_row && lane == 0) diag_in = __hip_atomic_load(&top_row[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  for (uint32_t s = 0; s < steps; ++s) {
    const uint32_t t = s & 63u;
    if (t == 0) {                       // refill the column-character window (coalesced 64 B)
      const uint32_t j = s + lane;
      chunk = j < nc ? cols.at(j) : PAD_COL;
      if (top_row) tchunk = j < nc ? __hip_atomic_load(&top_row[j + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    }
    uint32_t in = wave_shr1(out);
    const uint32_t ch0 = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)t);
    const uint32_t top_in = (uint32_t)__builtin_amdgcn_readlane((int)tchunk, (int)t);
    if (lane == 0) {
      uint32_t top = top_row ? top_in : s + 1;             // M[row_base][j], j = s+1
      if constexpr (BAND) { if (!top_row && top > band_k) top = BAND_INF; }
      in = top | (ch0 << 24);
    }
    const uint32_t j = s - lane + 1;                     // column of this lane (wraps when idle)
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
        lev_cell<R, WILD, DIRS, ROWMIN, AFFIX, BAND, ASMALL>(r, rc[r], ch, ch_n, diag, up, cur[r], minv[r], minpos[r], best, dp,
                                                             row_base + row0 + r + 1, j, band_k);
      diag_in = in_val;
      out = up | (ch << 24);
      if constexpr (DIRS) dp.store(dir_ws + ((size_t)s * 64 + lane) * EB);
      if (bottom_row && lane == last_lane) {
        uint32_t bv = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) if ((uint32_t)r == last_r) bv = cur[r];
        __hip_atomic_store(&bottom_row[j], bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// One column sweep over at most 64*R rows (the common case; strips of longer jobs: lev_sweep_strip).
// The step loop is a chain of dependent instructions on one wave, so each instruction in it is
// latency: per 64-step chunk the inputs of lane 0 (top value | column character) are prepared by
// all lanes at once in ONE register (`feed`, lane t = step t) that moves one lane down per step, so
// lane 0 always holds the input of the current step and the DPP shift that passes the strips' last
// rows along drops it in: two DPP moves per step, no scalar round trip.  On return
// cur[r] = M[row(l,r)][nc].
template <int R, bool WILD, bool DIRS, bool ROWMIN, bool AFFIX, bool BAND = false, bool ASMALL = false>
__device__ __forceinline__ void lev_sweep(const Operand rows, const uint32_t nr,
                                          const Operand cols, const uint32_t nc,
                                          const uint32_t lane, uint32_t (&cur)[R],
                                          uint32_t (&minv)[R], uint32_t (&minpos)[R],
                                          AffixBest& best, uint8_t* dir_ws, const uint32_t band_k = 0) {
  uint32_t rc[R];                       // row characters of this lane's strip
  const uint32_t row0 = lane * R;       // rows row0+1 .. row0+R
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = row0 + r;
    rc[r] = i < nr ? rows.at(i) : PAD_ROW;
    cur[r] = i + 1;                     // M[i+1][0]
    if constexpr (BAND) { if (i + 1 > band_k) cur[r] = BAND_INF; }
    if constexpr (ROWMIN) { minv[r] = i + 1; minpos[r] = 0; }
  }
  if (nr == 0 || nc == 0) return;
  const uint32_t last_lane = (nr - 1) / R;
  const uint32_t steps = nc + last_lane;
  uint32_t diag_in = row0;              // M[row0][j-1] for j = 1
  uint32_t out = 0;                     // (value of the strip's last row) | (column char << 24)
  constexpr uint32_t EB = R <= 4 ? 1u : R / 4;

  // the column characters of chunk c+1 are requested while chunk c is swept (the load would otherwise sit
  // at the head of every chunk's dependent chain: ~1 us of L2/HBM latency per 64 steps)
  auto feed_of = [&](const uint32_t s0) -> uint32_t {
    const uint32_t jc = s0 + lane;      // column jc+1 enters lane 0 at step jc
    uint32_t top = jc + 1u;             // M[0][jc+1]
    if constexpr (BAND) { if (top > band_k) top = BAND_INF; }
    return top | ((jc < nc ? cols.at(jc) : PAD_COL) << 24);
  };
  uint32_t feed_next = feed_of(0);
  for (uint32_t s0 = 0; s0 < steps; s0 += 64) {
    uint32_t feed = feed_next;
    feed_next = feed_of(s0 + 64u);
    const uint32_t tmax = (min(64u, steps - s0) + 7u) & ~7u;   // whole groups of 8; steps past the end touch no cell
    for (uint32_t t0 = 0; t0 < tmax; t0 += 8) {
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t s = s0 + t0 + u;
        const uint32_t in = wave_shr1_first(feed, out);
        feed = wave_shl1(feed);
        const uint32_t j = s - lane + 1;                   // column of this lane (wraps when idle)
        if (j - 1u < nc) {
          const uint32_t ch = in >> 24;
          const uint32_t in_val = in & 0xFFFFFFu;
          uint32_t up = in_val;
          uint32_t diag = diag_in;
          const bool ch_n = WILD && is_n(ch);
          DirPack<R> dp;
          if constexpr (DIRS) dp.clear();
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const uint32_t left = cur[r];
            bool match = rc[r] == ch;
            if constexpr (WILD) match = match || ch_n || is_n(rc[r]);
            uint32_t v = diag + (match ? 0u : 1u);
            if constexpr (DIRS) {
              // ComputeAlignMatrix tie-break: diagonal, then up (dir 1), then left (dir 2), strict >
              uint32_t d = 0;
              if (v > up + 1) { v = up + 1; d = 1; }
              if (v > left + 1) { v = left + 1; d = 2; }
              dp.set(r, d);
            } else {
              v = min(v, min(up + 1, left + 1));
            }
            if constexpr (BAND) {
              // K_band_edit_distance keeps cells with |column - row| <= k only; neighbours outside
              // the band do not take part in the minimum (src/compute-alignments.c:375-443)
              const uint32_t row = row0 + r + 1;
              v = (j + band_k >= row && row + band_k >= j) ? min(v, BAND_INF) : BAND_INF;
            }
            if constexpr (ROWMIN) {
              if (minv[r] > v) { minv[r] = v; minpos[r] = j; }   // strict: first arg-min
            }
            if constexpr (AFFIX) {
              // cut_weight = 2*v/(e+g) <= 0.17  <=>  200*v <= 17*(e+g)   (exact)
              best.template consider<ASMALL>(rc[r] == ch, v, row0 + r + 1, j);
            }
            diag = left;
            cur[r] = v;
            up = v;
          }
          diag_in = in_val;
          out = up | (ch << 24);
          if constexpr (DIRS) dp.store(dir_ws + ((size_t)s * 64 + lane) * EB);
        }
      }
    }
  }
}

// value of row `row` (1-based) after a sweep, written by the lane that owns it (predicated
// stores instead of a dynamically indexed register array)
template <int R>
__device__ __forceinline__ void store_row_value(const uint32_t (&a)[R], uint32_t lane, uint32_t row,
                                                int32_t* dst) {
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (lane * R + r + 1 == row) *dst = (int32_t)a[r];
}

enum { MODE_ED = 0, MODE_ALIGN = 1, MODE_BORDERS = 2, MODE_AFFIX = 3, MODE_KBAND = 4 };

// MODE_ED      edit_distance last cell (src/refine.c:50-83) / compute_edit_distance
//              (src/compute-alignments.c:240-249)
// MODE_ALIGN   ComputeAlignMatrix (src/compute-alignments.c:85-147) incl. the equal-string
//              shortcut of compute_alignment (:48-58); directions go to the workspace
// MODE_BORDERS general_refine_borders (src/refine.c:105-192)
// MODE_AFFIX   find_longest_affix (src/factorization-refinement.c:1136-1173)
// STRIPS (R = 64 only): jobs with more than 4096 rows, swept in strips of 4096 rows; the job's
// workspace starts with the two boundary rows (strip_bnd_bytes each), ALIGN directions follow,
// one block of (columns + 64) * 64 * 16 bytes per strip.

// dustScore (src/exon-complexity.c:50-78) of s[0..len) on one wave: every dinucleotide adds the number of times it has
// been seen before, i.e. the sum over the 17 dinucleotide classes (getDinucleotideIndex :80-130: A, C, G, T in either
// case, everything else class 16) of f (f - 1) / 2 for their final counts f -- an integer, so the FP64 arithmetic that
// follows (x 10.0, / (length - 2), / length) sees the reference's running total.  The counts come from ballots over 64
// positions at a time.  Same value in every lane.
__device__ __noinline__ double dust_score_wave(const uint8_t* __restrict__ s, const uint32_t len, const uint32_t lane) {
  if ((int)len <= 2) return 0.0;
  uint32_t cnt[17];
#pragma unroll
  for (int b = 0; b < 17; ++b) cnt[b] = 0u;
  const uint32_t nd = len - 1u;                  // dinucleotides
  for (uint32_t base = 0; base < nd; base += 64u) {
    const uint32_t i = base + lane;
    int cls = -1;                                // no dinucleotide on this lane
    if (i < nd) {
      const int x = acgt_code(s[i]), y = acgt_code(s[i + 1]);
      cls = (x < 0 || y < 0) ? 16 : 4 * x + y;
    }
#pragma unroll
    for (int b = 0; b < 17; ++b) cnt[b] += (uint32_t)__popcll(__ballot(cls == b));
  }
  unsigned long long running = 0ull;
#pragma unroll
  for (int b = 0; b < 17; ++b) running += (unsigned long long)cnt[b] * (cnt[b] - (cnt[b] ? 1u : 0u)) / 2ull;
  const double dust = (10.0 * (double)running) / ((double)(len - 2u));
  return dust / (double)len;
}
// the exon check's flags (pgpu_gpu.h: KBAND with tail = 1): bit 0 dust(a) > threshold, bit 1 dust(b) > threshold
__device__ __forceinline__ uint32_t dust_flags_wave(const DevJob& job, const uint32_t lane) {
  const double thr = __longlong_as_double((long long)(((unsigned long long)job.p2 << 32) | (unsigned long long)job.p1));
  const double da = dust_score_wave(job.a, job.la, lane), db = dust_score_wave(job.b, job.lb, lane);
  return (da > thr ? 1u : 0u) | (db > thr ? 2u : 0u);
}

// K_band_edit_distance (src/compute-alignments.c:375-443) with THE BAND ON THE LANES: lane s owns
// slot s of the reference's 2k+1 wide row buffers, i.e. the diagonal column - row = s - k, and the
// wave walks down the rows.  Cell (r, s) needs (r-1, s) [diagonal: the lane's own previous value],
// (r-1, s+1) [up: the right neighbour's previous row] and (r, s-1) [left: the left neighbour's same
// row], so lane s takes row r at time 2r + s: even lanes in the first half of an iteration, odd
// lanes in the second, each reading its neighbours' latest value over DPP.  m + k iterations of two
// single-cell half-steps instead of (n + 63) steps of R cells on the matrix sweep.  Needs 2k+1 <= 64.
// A lane works on the rows whose column lies in 1..n; before its first row it holds the boundary
// value next to it -- M[0][s-k] = s-k for the slots right of the main diagonal, M[k-s][0] = k-s for
// those left of it -- which is what its right neighbour reads as "left" and itself as "diagonal"
// on its first row.  Slot 0 has no left term and slot 2k no up term, as in the reference's loops.
__device__ __noinline__ void kband_band_sweep(const uint8_t* __restrict__ lng, const uint32_t n,
                                              const uint8_t* __restrict__ sht, const uint32_t m,
                                              const uint32_t k, const uint32_t lane, DevResult* res) {
  const uint32_t W = 2u * k + 1u;
  const bool used = lane < W;
  const bool odd = (lane & 1u) != 0u;
  const int off = (int)lane - (int)k;            // column - row on this lane's diagonal
  const uint32_t half = lane >> 1;               // iteration q works on row r = q - half
  // neighbours that do not exist are pushed out of the minimum
  const uint32_t up_mask = (lane + 1u < W) ? 0u : BAND_INF, left_mask = lane > 0u ? 0u : BAND_INF;
  uint32_t val = (uint32_t)(off < 0 ? -off : off);
  // rows of this lane: 1 <= r <= m with 1 <= off + r <= n
  const uint32_t r_lo = off < 0 ? (uint32_t)(1 - off) : 1u;
  const int hi_i = (int)n - off < (int)m ? (int)n - off : (int)m;
  const uint32_t span = (used && hi_i >= (int)r_lo) ? (uint32_t)hi_i - r_lo : 0xFFFFFFFFu;   // r - r_lo <= span: active
  const bool any_row = used && hi_i >= (int)r_lo;
  const uint32_t nq = m + k;
  // characters of the cell of iteration q (the loads run a group of four iterations ahead)
  auto row_char = [&](uint32_t q) -> uint32_t {
    const uint32_t r = q - half;
    return (any_row && r - r_lo <= span) ? (uint32_t)sht[r - 1u] : 0u;
  };
  auto col_char = [&](uint32_t q) -> uint32_t {
    const uint32_t r = q - half;
    return (any_row && r - r_lo <= span) ? (uint32_t)lng[(uint32_t)(off + (int)r) - 1u] : 1u;
  };
  uint32_t a[4], b[4], an[4], bn[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { a[j] = row_char(1u + j); b[j] = col_char(1u + j); }
  for (uint32_t q0 = 1; q0 <= nq; q0 += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { an[j] = row_char(q0 + 4u + j); bn[j] = col_char(q0 + 4u + j); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t r = q0 + j - half;          // wraps for the lanes whose first row lies ahead
      const bool active = any_row && (r - r_lo <= span);
      const uint32_t mism = a[j] != b[j] ? 1u : 0u;
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const uint32_t upv = wave_shl1(val) | up_mask, leftv = wave_shr1(val) | left_mask;
        const uint32_t nv = min(val + mism, min(upv, leftv) + 1u);
        val = (active && odd == (par == 1)) ? nv : val;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] = an[j]; b[j] = bn[j]; }
  }
  if (lane == n + k - m) { res->status = 0; res->v[1] = (int32_t)val; res->v[0] = val <= k ? 1 : 0; }
}

template <int R, int MODE, bool STRIPS = false>
__device__ __forceinline__ void lev_wave_body(const DevJob& job, DevResult* res, uint8_t* __restrict__ ws,
                                              const uint32_t lane, uint32_t* wave_lds = nullptr) {
  uint32_t cur[R], minv[R], minpos[R];
  AffixBest best = AFFIX_NONE;

  if constexpr (MODE == MODE_ED) {
    // distance is symmetric: keep the shorter string on the rows
    const bool swap = job.la > job.lb;
    const Operand rows{swap ? job.b : job.a, 0, false}, cols{swap ? job.a : job.b, 0, false};
    const uint32_t nr = swap ? job.lb : job.la, nc = swap ? job.la : job.lb;
    if constexpr (STRIPS) {
      constexpr uint32_t SR = 64u * R;
      uint32_t* bnd = reinterpret_cast<uint32_t*>(ws + job.ws_off);
      const size_t bw = strip_bnd_bytes(nc) / 4;
      uint32_t done = 0;
      for (uint32_t k = 0; done < nr; ++k, done += SR) {
        const uint32_t part = min(SR, nr - done);
        const Operand rs{rows.base + done, 0, false};
        lev_sweep_strip<R, false, false, false, false>(rs, part, cols, nc, lane, cur, minv, minpos, best, nullptr, 0, done,
                                                 k ? bnd + ((k - 1) & 1) * bw : nullptr, done + part < nr ? bnd + (k & 1) * bw : nullptr);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the next strip reads this strip's last row
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      store_row_value<R>(cur, lane, nr - (done - SR), &res->v[0]);
      if (lane == 0) res->status = 0;
      return;
    }
    lev_sweep<R, false, false, false, false>(rows, nr, cols, nc, lane, cur, minv, minpos, best, nullptr);
    if (nr == 0) { if (lane == 0) { res->status = 0; res->v[0] = (int32_t)nc; } return; }
    store_row_value<R>(cur, lane, nr, &res->v[0]);
    if (lane == 0) res->status = 0;
  } else if constexpr (MODE == MODE_ALIGN) {
    const uint32_t n = job.la, m = job.lb;
    bool same = n == m;
    if (same) for (uint32_t i = lane; i < n; i += 64) same = same && job.a[i] == job.b[i];
    if (__all(same)) {                   // identity alignment, score 0 (compute-alignments.c:48-58)
      if (lane == 0) { res->status = 0; res->v[0] = 0; res->v[1] = (int32_t)n; res->v[5] = 1; }
      return;
    }
    const Operand rows{job.a, 0, false}, cols{job.b, 0, false};
    if constexpr (STRIPS) {
      constexpr uint32_t SR = 64u * R;
      uint32_t* bnd = reinterpret_cast<uint32_t*>(ws + job.ws_off);
      const size_t bw = strip_bnd_bytes(m) / 4;
      uint8_t* dirs = ws + job.ws_off + 2 * strip_bnd_bytes(m);
      const size_t strip_dirs = ((size_t)m + 64) * 64 * (R / 4);
      uint32_t done = 0;
      for (uint32_t k = 0; done < n; ++k, done += SR) {
        const uint32_t part = min(SR, n - done);
        const Operand rs{job.a + done, 0, false};
        lev_sweep_strip<R, true, true, false, false>(rs, part, cols, m, lane, cur, minv, minpos, best, dirs + k * strip_dirs, 0, done,
                                               k ? bnd + ((k - 1) & 1) * bw : nullptr, done + part < n ? bnd + (k & 1) * bw : nullptr);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the next strip reads this strip's last row
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      store_row_value<R>(cur, lane, n - (done - SR), &res->v[0]);
      if (lane == 0) { res->status = 0; res->v[5] = 0; }
      return;
    }
    lev_sweep<R, true, true, false, false>(rows, n, cols, m, lane, cur, minv, minpos, best, ws + job.ws_off);
    if (n == 0 || m == 0) { if (lane == 0) { res->status = 0; res->v[0] = (int32_t)(n + m); res->v[5] = 0; } return; }
    store_row_value<R>(cur, lane, n, &res->v[0]);
    if (lane == 0) { res->status = 0; res->v[5] = 0; }
  } else if constexpr (MODE == MODE_BORDERS) {
    const uint32_t len_p = job.la, len_t = job.lb, max_errs = job.p2;
    const uint32_t t_win = min(len_p + max_errs, len_t);
    const BordersMins mins{wave_lds, len_p};       // the wave's own LDS region (several jobs per workgroup)
    {
      const Operand rows{job.a, len_p, false}, cols{job.b, len_t, false};
      lev_sweep<R, false, false, true, false>(rows, len_p, cols, t_win, lane, cur, minv, minpos, best, nullptr);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t i = lane * R + r + 1;
        if (i <= len_p) { mins.pre[i] = minv[r]; mins.pre_pos[i] = minpos[r]; }
      }
    }
    {
      const Operand rows{job.a, len_p, true}, cols{job.b, len_t, true};
      lev_sweep<R, false, false, true, false>(rows, len_p, cols, t_win, lane, cur, minv, minpos, best, nullptr);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t i = lane * R + r + 1;
        if (i <= len_p) { mins.suf[i] = minv[r]; mins.suf_pos[i] = minpos[r]; }
      }
    }
    if (lane == 0) { mins.pre[0] = 0; mins.pre_pos[0] = 0; mins.suf[0] = 0; mins.suf_pos[0] = 0; }
    // one wave produced the four arrays and one wave reads them: a wave-level hand-over (a workgroup
    // barrier would couple this wave to the unrelated jobs of its neighbours)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    borders_cut_scan(job, res, lane, mins.pre, mins.pre_pos, mins.suf, mins.suf_pos);
  } else if constexpr (MODE == MODE_KBAND) {
    // K_band_edit_distance (src/compute-alignments.c:319-453): early exits in the reference's
    // order, then the banded DP (or the full matrix when 2k+1 >= n, :370-373).  rows = shorter.
    if (job.tail != 0u) {                                    // exon check: the two dust comparisons beside the distance
      const uint32_t fl = dust_flags_wave(job, lane);
      if (lane == 0) res->v[2] = (int32_t)fl;
    }
    const uint32_t ub = job.p0;
    const bool swap = job.la < job.lb;                       // reference: seq1 becomes the longer
    const uint8_t* lng = swap ? job.b : job.a; const uint8_t* sht = swap ? job.a : job.b;
    const uint32_t n = swap ? job.lb : job.la, m = swap ? job.la : job.lb;
    bool same = n == m;
    if (same) for (uint32_t i = lane; i < n; i += 64) same = same && lng[i] == sht[i];
    same = __all(same);
    if (same || ub == 0 || n - m > ub) {
      if (lane == 0) {
        res->status = 0;
        if (same) { res->v[0] = 1; res->v[1] = 0; }
        else if (ub == 0) { res->v[0] = 0; res->v[1] = 1; }
        else { res->v[0] = 0; res->v[1] = (int32_t)(n - m); }
      }
      return;
    }
    const bool banded = !(2ull * ub + 1 >= n);
    if (banded && 2u * ub + 1u <= 64u) { kband_band_sweep(lng, n, sht, m, ub, lane, res); return; }
    const Operand rows{sht, 0, false}, cols{lng, 0, false};
    if constexpr (STRIPS) {
      constexpr uint32_t SR = 64u * R;
      uint32_t* bnd = reinterpret_cast<uint32_t*>(ws + job.ws_off);
      const size_t bw = strip_bnd_bytes(n) / 4;
      uint32_t done = 0;
      for (uint32_t k = 0; done < m; ++k, done += SR) {
        const uint32_t part = min(SR, m - done);
        const Operand rs{sht + done, 0, false};
        const uint32_t* tp = k ? bnd + ((k - 1) & 1) * bw : nullptr;
        uint32_t* bt = done + part < m ? bnd + (k & 1) * bw : nullptr;
        if (banded) lev_sweep_strip<R, false, false, false, false, true>(rs, part, cols, n, lane, cur, minv, minpos, best, nullptr, ub, done, tp, bt);
        else        lev_sweep_strip<R, false, false, false, false, false>(rs, part, cols, n, lane, cur, minv, minpos, best, nullptr, 0, done, tp, bt);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the next strip reads this strip's last row
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      const uint32_t lrow = m - (done - SR);
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (lane * R + r + 1 == lrow) { res->status = 0; res->v[1] = (int32_t)cur[r]; res->v[0] = cur[r] <= ub ? 1 : 0; }
      return;
    }
    if (banded) lev_sweep<R, false, false, false, false, true>(rows, m, cols, n, lane, cur, minv, minpos, best, nullptr, ub);
    else        lev_sweep<R, false, false, false, false, false>(rows, m, cols, n, lane, cur, minv, minpos, best, nullptr);
    if (m == 0) { if (lane == 0) { res->status = 0; res->v[1] = (int32_t)n; res->v[0] = n <= ub ? 1 : 0; } return; }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (lane * R + r + 1 == m) { res->status = 0; res->v[1] = (int32_t)cur[r]; res->v[0] = cur[r] <= ub ? 1 : 0; }
  } else {  // MODE_AFFIX
    const Operand rows{job.a, 0, false}, cols{job.b, 0, false};
    if constexpr (STRIPS) {
      constexpr uint32_t SR = 64u * R;
      uint32_t* bnd = reinterpret_cast<uint32_t*>(ws + job.ws_off);
      const size_t bw = strip_bnd_bytes(job.lb) / 4;
      uint32_t done = 0;
      for (uint32_t k = 0; done < job.la; ++k, done += SR) {
        const uint32_t part = min(SR, job.la - done);
        const Operand rs{job.a + done, 0, false};
        lev_sweep_strip<R, false, false, false, true>(rs, part, cols, job.lb, lane, cur, minv, minpos, best, nullptr, 0, done,
                                                k ? bnd + ((k - 1) & 1) * bw : nullptr, done + part < job.la ? bnd + (k & 1) * bw : nullptr);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the next strip reads this strip's last row
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
    } else if (job.la + job.lb < 32768u) {
      lev_sweep<R, false, false, false, true, false, true>(rows, job.la, cols, job.lb, lane, cur, minv, minpos, best, nullptr);
    } else {
      lev_sweep<R, false, false, false, true>(rows, job.la, cols, job.lb, lane, cur, minv, minpos, best, nullptr);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {       // wave-wide arg-best
      const AffixBest o = best.from_lane_xor(off);
      if (o.s && best.worse_than(o)) best = o;
    }
    if (lane == 0) {
      res->status = 0; res->v[0] = (int32_t)best.valid();
      res->v[1] = (int32_t)best.e(); res->v[2] = (int32_t)best.g();
    }
  }
}

// TracebackAlignment (src/compute-alignments.c:149-207), one WAVE per job.
// The walk from (n,m) back to the border is a chain of dependent direction look-ups; done by one
// thread against HBM/L2 every step costs a memory round trip (~250 ns).  Here the wave copies a
// window of direction entries (a run of consecutive sweep steps, coalesced 16 B per lane) into
// LDS and walks it there; the walk state is wave-uniform, so it lives in scalar registers and a
// step is one LDS read plus a few scalar instructions.  The walk only records the 2-bit
// direction per step; the gapped strings are then written by all 64 lanes at once: the character
// a step consumes is found from a prefix count (ballot + popcount) of the steps before it.


__device__ __forceinline__ void align_traceback_wave(const DevJob& job, DevResult* res, const uint8_t* __restrict__ ws,
                                                     uint8_t* __restrict__ strs, const uint32_t lane,
                                                     uint8_t* win, uint8_t* path) {
  // the walk is wave-uniform: its state has to be uniform for the compiler too (scalar registers and
  // branches instead of per-lane values under an exec mask: a third of the instructions per step)
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.la), m = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.lb), cap = n + m + 1;
  uint8_t* ea = strs + job.str_off;
  uint8_t* ga = ea + cap;
  if (res->v[5] == 1) {                  // identity alignment
    for (uint32_t i = lane; i < n; i += 64) { ea[i] = job.a[i]; ga[i] = job.b[i]; }
    if (lane == 0) {
      ea[n] = 0; ga[n] = 0;
      res->v[1] = (int32_t)n;
      res->str[0] = job.str_off; res->str[1] = job.str_off + cap;
      res->v[5] = 0;
    }
    return;
  }
  const uint32_t rcls = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.r_class);
  const bool strips = rcls == ROW_CLASS_STRIPS;            // more than 4096 rows: strips of 64*64 rows
  const uint32_t R = strips ? 64u : rcls, EB = R <= 4 ? 1u : R / 4;
  const uint32_t lgR = 31u - (uint32_t)__builtin_clz(R);   // R is a power of two
  const uint32_t WS = TB_WIN_BYTES / (64u * EB);           // sweep steps per window
  const uint8_t* dirs = ws + job.ws_off + (strips ? 2 * strip_bnd_bytes(m) : 0);
  const size_t strip_dirs = ((size_t)m + 64) * 64 * EB;
  uint32_t i = n, j = m, k = 0, np = 0;
  uint32_t i0 = n, j0 = m, pos = cap - 1;
  if (lane == 0) { ea[pos] = 0; ga[pos] = 0; }
  uint32_t s_lo = 1u, s_hi = 0u, win_strip = 0;            // empty window
  while (i > 0 && j > 0) {
    const uint32_t strip = strips ? (i - 1) >> 12 : 0u, li = strips ? (i - 1) & 4095u : i - 1;
    const uint32_t l = li >> lgR, r = li & (R - 1), s = (j - 1) + l;
    if (s < s_lo || s > s_hi || strip != win_strip) {      // bring in the steps (s - WS, s] of the strip
      s_hi = s; s_lo = s + 1 >= WS ? s + 1 - WS : 0; win_strip = strip;
      const uint32_t bytes = (s_hi - s_lo + 1) * 64u * EB;
      const uint8_t* src = dirs + strip * strip_dirs + (size_t)s_lo * 64u * EB;
      for (uint32_t off = lane * 16u; off < bytes; off += 64u * 16u)
        *reinterpret_cast<uint4*>(win + off) = *reinterpret_cast<const uint4*>(src + off);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    uint32_t d = (win[((s - s_lo) * 64u + l) * EB + (r >> 2)] >> (2u * (r & 3u))) & 3u;
    d = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);  // the walk is wave-uniform: keep it scalar
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
  // what is left of one string is aligned to gaps (:193-206): a[..i) over '-', then '-' over b[..j)
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

// ---------------------------------------------------------------------------------------------
// ComputeAlignMatrix + TracebackAlignment (src/compute-alignments.c:85-207) inside a BAND, on one wave.
// An exon and its stretch of the genomic sequence differ by a few per cent, so the alignment lies next to
// the main diagonal.  Lane s owns the diagonal column - row = s - k (k = ALIGN_BAND_K, 2k+1 <= 64) and the
// wave walks down the rows exactly as kband_band_sweep does (lane s takes row r at time 2r + s; diagonal =
// its own previous value, up = the right neighbour's previous row, left = the left neighbour's same row),
// with the N wildcard and the reference's preference diagonal < up < left recorded per cell.
// Why the answer is the full matrix's: M[i][j] >= |i - j|, so a cell whose true value is <= k lies inside
// the band together with every optimal path that ends in it -- its banded value is the true one; a cell
// with a true value > k gets a banded value >= the true one, hence > k.  If the banded M[n][m] is <= k it
// is the true score, every cell of the reference's traceback has a value <= the score, and at such a cell
// the candidates that reach the minimum have true (= banded) neighbour values, all others are larger in
// both matrices (a neighbour outside the band is worth >= k + 1): the same first minimum in the order
// diagonal, up, left, i.e. the same direction.  A banded score > k says nothing: the caller sweeps the
// whole matrix.  Directions: 2 bits per cell, one 32-bit word per lane and 16 rows, [row / 16][lane].
// ---------------------------------------------------------------------------------------------
constexpr uint32_t ALIGN_BAND_K = ALIGN_BAND_HALF;

// returns the banded M[n][m] in every lane; dirs: ((n >> 4) + 1) * 64 words
__device__ __noinline__ uint32_t align_band_sweep(const uint8_t* __restrict__ a, const uint32_t n,
                                                  const uint8_t* __restrict__ b, const uint32_t m,
                                                  const uint32_t lane, uint32_t* __restrict__ dirs) {
  constexpr uint32_t k = ALIGN_BAND_K, W = 2u * k + 1u;
  const bool used = lane < W;
  const bool odd = (lane & 1u) != 0u;
  const int off = (int)lane - (int)k;            // column - row on this lane's diagonal
  const uint32_t half = lane >> 1;               // iteration q works on row r = q - half
  const uint32_t up_mask = (lane + 1u < W) ? 0u : BAND_INF, left_mask = lane > 0u ? 0u : BAND_INF;
  uint32_t val = (uint32_t)(off < 0 ? -off : off);
  // rows of this lane: 1 <= r <= n with 1 <= r + off <= m
  const uint32_t r_lo = off < 0 ? (uint32_t)(1 - off) : 1u;
  const int hi_i = (int)m - off < (int)n ? (int)m - off : (int)n;
  const bool any_row = used && hi_i >= (int)r_lo;
  const uint32_t span = any_row ? (uint32_t)hi_i - r_lo : 0xFFFFFFFFu;   // r - r_lo <= span: active
  const uint32_t nq = n + k;                     // lane 2k takes row n in iteration n + k
  auto row_char = [&](uint32_t q) -> uint32_t {
    const uint32_t r = q - half;
    return (any_row && r - r_lo <= span) ? (uint32_t)a[r - 1u] : 0u;
  };
  auto col_char = [&](uint32_t q) -> uint32_t {
    const uint32_t r = q - half;
    return (any_row && r - r_lo <= span) ? (uint32_t)b[(uint32_t)(off + (int)r) - 1u] : 1u;
  };
  uint32_t dw = 0u;                              // directions of the rows of the current group of 16
  uint32_t ca[4], cb[4], can[4], cbn[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { ca[j] = row_char(1u + j); cb[j] = col_char(1u + j); }
  for (uint32_t q0 = 1; q0 <= nq; q0 += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { can[j] = row_char(q0 + 4u + j); cbn[j] = col_char(q0 + 4u + j); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t r = q0 + j - half;          // wraps for the lanes whose first row lies ahead
      const bool active = any_row && (r - r_lo <= span);
      const uint32_t mism = (ca[j] == cb[j] || is_n(ca[j]) || is_n(cb[j])) ? 0u : 1u;
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const uint32_t upv = (wave_shl1(val) | up_mask) + 1u, leftv = (wave_shr1(val) | left_mask) + 1u;
        uint32_t nv = val + mism, d = 0u;
        if (nv > upv) { nv = upv; d = 1u; }
        if (nv > leftv) { nv = leftv; d = 2u; }
        const bool mine = active && odd == (par == 1);
        val = mine ? nv : val;
        dw |= mine ? d << (2u * (r & 15u)) : 0u;
      }
      // the word of rows 16 g .. 16 g + 15 is complete after row 16 g + 15, or after the lane's last row
      if (active && ((r & 15u) == 15u || r - r_lo == span)) { dirs[(r >> 4) * 64u + lane] = dw; dw = 0u; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { ca[j] = can[j]; cb[j] = cbn[j]; }
  }
  return (uint32_t)__shfl((int)val, (int)(m + k - n));
}

// the traceback over the band's directions (same walk, same output as align_traceback_wave)
__device__ __forceinline__ void align_band_traceback(const DevJob& job, DevResult* res, const uint32_t* __restrict__ dirs,
                                                     uint8_t* __restrict__ strs, const uint32_t lane,
                                                     uint8_t* win, uint8_t* path) {
  constexpr uint32_t k0 = ALIGN_BAND_K;
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.la), m = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.lb), cap = n + m + 1;
  uint8_t* ea = strs + job.str_off;
  uint8_t* ga = ea + cap;
  constexpr uint32_t WB = TB_WIN_BYTES / 256u;             // groups of 16 rows per window
  const uint32_t* w32 = reinterpret_cast<const uint32_t*>(win);
  uint32_t i = n, j = m, k = 0, np = 0;
  uint32_t i0 = n, j0 = m, pos = cap - 1;
  if (lane == 0) { ea[pos] = 0; ga[pos] = 0; }
  uint32_t g_lo = 1u, g_hi = 0u;                           // empty window (groups of 16 rows)
  while (i > 0 && j > 0) {
    const uint32_t g = i >> 4;
    if (g < g_lo || g > g_hi) {                            // bring in the groups (g - WB, g]
      g_hi = g; g_lo = g + 1 >= WB ? g + 1 - WB : 0;
      const uint32_t bytes = (g_hi - g_lo + 1) * 256u;
      const uint8_t* src = reinterpret_cast<const uint8_t*>(dirs) + (size_t)g_lo * 256u;
      for (uint32_t off = lane * 16u; off < bytes; off += 64u * 16u)
        *reinterpret_cast<uint4*>(win + off) = *reinterpret_cast<const uint4*>(src + off);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    uint32_t d = (w32[(g - g_lo) * 64u + (j + k0 - i)] >> (2u * (i & 15u))) & 3u;
    d = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);  // the walk is wave-uniform: keep it scalar
    path[np] = (uint8_t)d;
    ++np;
    i -= d < 2u ? 1u : 0u;                                 // 0: diagonal, 1: up, 2: left
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

// compute_maximum_edit_distance_for_exons (src/est-factorizations.c:1828-1840) of an exon of `len` genomic bytes, in FP64
// like the host
__device__ __forceinline__ uint32_t max_edit_for_exon(const uint32_t len) {
  const double rate = len > 100u ? 0.030 : (len > 50u ? 0.035 : 0.040);
  const double c = ceil((double)len * rate);
  return (uint32_t)(c > 1.0 ? c : 1.0);
}

// ---------------------------------------------------------------------------------------------
// The trimming walks of handle_endpoints (src/est-factorizations.c:2163-2196 head, :2231-2296 tail) over the two gapped
// rows of an end exon's alignment, 64 columns at a time: lane t of a window holds one column, and the ballots say where
// the rows agree (eq) and where the row of the EST (eg) or of the genomic sequence (gg) has a gap.  The state of a walk
// is carried from window to window by the caller: endpoint_epilogue looks at one window, clean_kernel at all of them.
// ---------------------------------------------------------------------------------------------
// head: the first `lim` columns of the window, from the left, until more than five matches in a row -- tested before the
// next column is read, so one column late.  cf / ce: characters of the EST / of the genomic sequence walked over.
__device__ __forceinline__ void head_walk_window(const unsigned long long eq, const unsigned long long eg, const unsigned long long gg,
                                                 const uint32_t lim, uint32_t& matches, uint32_t& cf, uint32_t& ce, bool& stop) {
  uint32_t j = 0;
  while (j < lim && !stop) {
    if (matches > 5u) stop = true;
    else {
      if (eq >> j & 1ull) { ++cf; ++ce; ++matches; }
      else { if (!(eg >> j & 1ull)) ++cf; if (!(gg >> j & 1ull)) ++ce; matches = 0; }
      ++j;
    }
  }
}
// tail: from column j down, in the window whose lane t holds column wb + t, until more than ten matches in a row.  cf / ce:
// the last character of the EST / of the genomic sequence not yet walked over.  false: the walk left the window running.
__device__ __forceinline__ bool tail_walk_window(const unsigned long long eq, const unsigned long long eg, const unsigned long long gg,
                                                 const uint32_t wb, int& j, uint32_t& matches, int& cf, int& ce, bool& stop) {
  while (j >= 0 && !stop) {
    if (matches > 10u) stop = true;
    else {
      if (j < (int)wb) return false;
      const uint32_t t = (uint32_t)j - wb;
      if (eq >> t & 1ull) { --cf; --ce; ++matches; }
      else { if (!(eg >> t & 1ull)) --cf; if (!(gg >> t & 1ull)) --ce; matches = 0; }
      --j;
    }
  }
  return true;
}
// tail, then (:2241-2281): the gap columns right of the run of matches are closed by pulling the next character of the
// gapped row over, as far as the characters agree.  Rows: e(q) / g(q) = the byte of a row at column q (0 behind the row),
// set_e / set_g rewrite one.
template <class Rows>
__device__ __forceinline__ void close_tail_gaps(Rows& rows, const uint32_t dim, uint32_t cursor, int& est_cl, int& gen_cl) {
  bool halt = false;
  while (!halt && cursor < dim - 1u) {
    const uint32_t ec = rows.e(cursor), gc = rows.g(cursor);
    if (!(ec == '-' || gc == '-')) break;
    uint32_t tr = cursor + 1u;
    if (ec == '-') {
      while (rows.e(tr) == '-') ++tr;
      const uint32_t moved = rows.e(tr);
      if (tr < dim && moved == gc) { rows.set_e(cursor, moved); rows.set_e(tr, '-'); ++est_cl; ++gen_cl; }
      else halt = true;
    } else {
      while (rows.g(tr) == '-') ++tr;
      const uint32_t moved = rows.g(tr);
      if (tr < dim && moved == ec) { rows.set_g(cursor, moved); rows.set_g(tr, '-'); ++est_cl; ++gen_cl; }
      else halt = true;
    }
    ++cursor;
  }
}

}  // namespace
