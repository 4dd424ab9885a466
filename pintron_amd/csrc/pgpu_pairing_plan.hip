// The pairing plan: a batch of patterns (ESTs) resident in HBM and the stages that run over them, one behind the other,
// without a result crossing the bus -- pairings, MEG records (pgpu_meg.hip), candidate factorizations (pgpu_cand.hip),
// factorizations (pgpu_fact.hip) -- and the pairing kernels, which replace
//   build_vertex_set (src/max-emb-graph.c:218-392)
// over the genomic index (pgpu_index.hip, read through PairIndexView).  Semantics (how the tree walk maps onto SA
// intervals, the suffix-link start rule, the two low-complexity filters) are stated in DESIGN.md section 4b and restated
// on the CPU, for the tests only, in oracle/pairing_oracle.c.  Everything per-EST is hand-written:
//   pair_locate   one wave per pattern, one lane per position: SA interval of the L-mer
//                 (two binary searches, T and SA are L2-resident: 9 B/base), then the longest
//                 match among the occurrences that are not preceded by P[i-1]
//   pair_chain    one thread per pattern: the sequential locus-depth recurrence
//                 D_i = max(A_i, s_i), threshold, next start depth from LCP-interval borders
//   pair_count / pair_fill / pair_cross / pair_emit
//                 per position: occurrences above the threshold, sort by t, filter (a);
//                 filter (b) against the previous position; compaction into (p,t,l) triples
#include <algorithm>
#include <cstdio>
#include <memory>
#include <new>

#include "pgpu_index.h"
#include "pgpu_stage_drive.h"
#include "pgpu_enum.h"
#include "pgpu_fact.h"
#include "pgpu_flists.h"
#include "pgpu_final.h"
#include "pgpu_unit.h"
#include "pgpu_side.h"
#include "pgpu_text.h"
#include "pgpu_small.h"
#include "pgpu_classify.h"

namespace {

// ---------------------------------------------------------------------------------------------
// pairings
// ---------------------------------------------------------------------------------------------
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct PairParams {
  uint32_t L;
  double rate;
};

// Sequences at 2 bits per base.  Both the genomic sequence and the patterns are compared sixteen bases per
// 32-bit word (one XOR and a count of trailing zeros) instead of a byte per load: a maximal pairing is as long
// as an exon, and pair_locate / pair_count / pair_fill walk it once per occurrence.  A flag bit per base marks
// what is not an upper-case A, C, G or T (N, the '*' and '#' that mask poly-A/T stretches, lower case): a
// window that holds a flagged base on either side is compared on the bytes, so the result is byte equality
// everywhere (an N equals an N, src/max-emb-graph.c compares characters).
struct PackedSeq { const uint32_t* __restrict__ code; const uint32_t* __restrict__ bad; };

__device__ __forceinline__ uint32_t pk_win16(const uint32_t* __restrict__ code, unsigned long long pos) {
  const unsigned long long w = pos >> 4;
  const unsigned long long x = ((unsigned long long)code[w + 1] << 32) | code[w];
  return (uint32_t)(x >> (2u * (uint32_t)(pos & 15u)));
}
__device__ __forceinline__ uint32_t pk_bad16(const uint32_t* __restrict__ bad, unsigned long long pos) {
  const unsigned long long w = pos >> 5;
  const unsigned long long x = ((unsigned long long)bad[w + 1] << 32) | bad[w];
  return (uint32_t)(x >> (uint32_t)(pos & 31u)) & 0xFFFFu;
}
// number of leading characters on which A[a..] and B[b..] agree, among the first `rem`
__device__ __forceinline__ uint32_t pk_match(const uint8_t* __restrict__ A, const PackedSeq Ap, unsigned long long a,
                                             const uint8_t* __restrict__ B, const PackedSeq Bp, unsigned long long b,
                                             uint32_t rem) {
  uint32_t l = 0;
  while (l < rem) {
    const uint32_t k = rem - l < 16u ? rem - l : 16u;
    const uint32_t mask = k < 16u ? (1u << k) - 1u : 0xFFFFu;
    if ((pk_bad16(Ap.bad, a + l) | pk_bad16(Bp.bad, b + l)) & mask) {
      uint32_t q = 0;
      while (q < k && A[a + l + q] == B[b + l + q]) ++q;
      l += q;
      if (q < k) break;
      continue;
    }
    uint32_t x = pk_win16(Ap.code, a + l) ^ pk_win16(Bp.code, b + l);
    if (k < 16u) x &= (1u << (2u * k)) - 1u;
    if (x) { l += (uint32_t)__builtin_ctz(x) >> 1; break; }
    l += k;
  }
  return l;
}

// what the comparisons of one pattern need: the genomic sequence and the pattern blob, as bytes and packed
struct CmpCtx {
  const uint8_t* __restrict__ T; PackedSeq Tp; uint32_t n;
  const uint8_t* __restrict__ pats; PackedSeq Pp;
};

// compare suffix t (from character `skip` on) with q[skip..d), q = pats + qabs: -1 / 0 (q[0..d) is a prefix) / +1.
// The caller guarantees the first `skip` characters are equal.
__device__ __forceinline__ int cmp_suffix(const CmpCtx& cx, uint32_t t, unsigned long long qabs, uint32_t d, uint32_t skip) {
  if (skip >= d) return 0;
  if (t + skip >= cx.n) return -1;                  // the suffix ended: it sorts first
  const uint32_t avail = cx.n - t - skip, want = d - skip;
  const uint32_t k = pk_match(cx.T, cx.Tp, (unsigned long long)t + skip, cx.pats, cx.Pp, qabs + skip, avail < want ? avail : want);
  if (k == want) return 0;
  if (k == avail) return -1;
  const uint32_t c = cx.T[t + skip + k], e = cx.pats[qabs + skip + k];
  return c < e ? -1 : 1;
}

// [lo,hi) of suffixes in sa[from,to) having q[0..d) as a prefix (all share q[0..skip))
__device__ void sa_interval(const CmpCtx& cx, const uint32_t* __restrict__ sa,
                            unsigned long long qabs, uint32_t d, uint32_t skip,
                            uint32_t from, uint32_t to, uint32_t* lo, uint32_t* hi) {
  uint32_t a = from, b = to;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (cmp_suffix(cx, sa[mid], qabs, d, skip) < 0) a = mid + 1; else b = mid;
  }
  *lo = a;
  b = to;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (cmp_suffix(cx, sa[mid], qabs, d, skip) <= 0) a = mid + 1; else b = mid;
  }
  *hi = a;
}

__device__ __forceinline__ bool prev_excluded(const uint8_t* __restrict__ T, uint32_t t,
                                              const uint8_t* __restrict__ P, uint32_t i) {
  return i > 0 && t > 0 && T[t - 1] == P[i - 1];     // src/max-emb-graph.c:178-181,195
}

// length of the match of P[i..m) with T[t..), known to be at least `from` (P = pats + pbase)
__device__ __forceinline__ uint32_t extend(const CmpCtx& cx, uint32_t t, unsigned long long pbase, uint32_t m, uint32_t i,
                                           uint32_t from) {
  if (i + from >= m || t + from >= cx.n) return from;
  const uint32_t rp = m - i - from, rt = cx.n - t - from;
  return from + pk_match(cx.T, cx.Tp, (unsigned long long)t + from, cx.pats, cx.Pp, pbase + i + from, rp < rt ? rp : rt);
}

// How many times the reference lists the occurrence t == 0 of position i (oracle/pairing_oracle.c
// states and tests the rule; src/max-emb-graph.c:168-216, src/aug_suffix_tree.c:183-192): suffix 0
// has no preceding character, sits in the slice of every symbol, and is reported once per slice walked
// -- through the unguarded loop where the child already reported holds an occurrence preceded by
// that symbol, through the guarded one (key 0, or key 1 next to the preceding symbol's key 0)
// elsewhere.  *l0 = lcp(P[i..], T[0..]); the result only matters when l0 reaches the threshold.
__device__ uint32_t zero_copies(const CmpCtx& cx, unsigned long long pbase, const uint32_t* __restrict__ sa,
                                const uint8_t* __restrict__ key, uint32_t sigma, const uint8_t* __restrict__ P,
                                uint32_t m, uint32_t i, uint32_t L, uint32_t lo, uint32_t hi, uint32_t l0) {
  const uint8_t* __restrict__ T = cx.T;
  unsigned long long present[4] = {0, 0, 0, 0};
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t t = sa[k];
    if (t == 0 || prev_excluded(T, t, P, i)) continue;
    if (extend(cx, t, pbase, m, i, L) > l0) { const uint32_t q = key[T[t - 1]]; present[q >> 6] |= 1ull << (q & 63u); }
  }
  const uint32_t sk = i > 0 ? key[P[i - 1]] : sigma;
  uint32_t copies = 0;
  for (uint32_t k = 0; k < sigma; ++k) {
    if (k == sk) continue;
    if ((present[k >> 6] >> (k & 63u)) & 1ull) ++copies;
    else if (k == 0 || (k == 1 && sk == 0)) ++copies;
  }
  return copies;
}

// one wave per pattern, lanes stride over its positions
__global__ __launch_bounds__(64)
void pair_locate_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint32_t* __restrict__ sa,
                        const uint32_t* __restrict__ klo, const uint32_t* __restrict__ khi,
                        const uint8_t* __restrict__ pats, const unsigned long long* __restrict__ pat_off,
                        PairParams prm, uint32_t* __restrict__ lo_out, uint32_t* __restrict__ hi_out,
                        uint32_t* __restrict__ a_out, const PackedSeq Tp, const PackedSeq Pp) {
  const CmpCtx cx{T, Tp, n, pats, Pp};
  const unsigned long long base = pat_off[blockIdx.x];
  const uint32_t m = (uint32_t)(pat_off[blockIdx.x + 1] - base);
  const uint8_t* P = pats + base;
  for (uint32_t i = threadIdx.x; i < m; i += 64) {
    uint32_t lo = 0, hi = 0, A = 0;
    if (m - i >= prm.L) {
      const int code = prm.L >= KTAB ? kmer_code(P + i, m - i) : -1;
      if (code >= 0) {                              // the k-mer's run, then bisect on characters KTAB..L
        const uint32_t from = klo[code], to = khi[code];
        if (from < to) sa_interval(cx, sa, base + i, prm.L, KTAB, from, to, &lo, &hi);
      } else {
        sa_interval(cx, sa, base + i, prm.L, 0, 0, n, &lo, &hi);
      }
      for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t t = sa[k];
        if (prev_excluded(T, t, P, i)) continue;
        const uint32_t l = extend(cx, t, base, m, i, prm.L);
        A = l > A ? l : A;
      }
    }
    lo_out[base + i] = lo; hi_out[base + i] = hi; a_out[base + i] = A;
  }
}

// one thread per pattern: the locus-depth recurrence (sequential in i)
__global__ __launch_bounds__(64)
void pair_chain_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint32_t* __restrict__ sa,
                       const uint32_t* __restrict__ lcp, const uint8_t* __restrict__ pats,
                       const unsigned long long* __restrict__ pat_off, uint32_t n_pat, PairParams prm,
                       const uint32_t* __restrict__ lo_in, const uint32_t* __restrict__ hi_in,
                       const uint32_t* __restrict__ a_in, uint32_t* __restrict__ thr_out, const PackedSeq Tp, const PackedSeq Pp) {
  const CmpCtx cx{T, Tp, n, pats, Pp};
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pat) return;
  const unsigned long long base = pat_off[p];
  const uint32_t m = (uint32_t)(pat_off[p + 1] - base);
  const uint8_t* P = pats + base;
  uint32_t s = 0;
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t A = a_in[base + i];
    const uint32_t D = A > s ? A : s;
    if (D < prm.L) { thr_out[base + i] = NONE; s = 0; continue; }
    const double scaled = (double)D * prm.rate;                  // src/max-emb-graph.c:273-274
    const double thr_d = scaled > (double)prm.L ? scaled : (double)prm.L;
    thr_out[base + i] = (uint32_t)thr_d;
    const uint32_t lo = lo_in[base + i], hi = hi_in[base + i];
    uint32_t l2 = lo, h2 = hi;
    if (hi - lo > 1 && D > prm.L) sa_interval(cx, sa, base + i, D, prm.L, lo, hi, &l2, &h2);
    const uint32_t pl = lcp[l2], ph = lcp[h2];
    const uint32_t par = pl > ph ? pl : ph;
    if (par == 0) { s = 0; continue; }
    bool at_node = false;
    if (h2 - l2 >= 2) {
      const uint32_t t1 = sa[l2], t2 = sa[h2 - 1];
      const int c1 = t1 + D < n ? (int)T[t1 + D] : -1;
      const int c2 = t2 + D < n ? (int)T[t2 + D] : -1;
      at_node = c1 != c2;
    }
    s = at_node ? D - 1 : par - 1;
  }
}

// number of occurrences at or above the threshold (before the filters)
__global__ __launch_bounds__(64)
void pair_count_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint32_t* __restrict__ sa,
                       const uint8_t* __restrict__ key, uint32_t sigma,
                       const uint8_t* __restrict__ pats, const unsigned long long* __restrict__ pat_off,
                       PairParams prm, const uint32_t* __restrict__ lo_in, const uint32_t* __restrict__ hi_in,
                       const uint32_t* __restrict__ thr_in, uint32_t* __restrict__ cnt_out, const PackedSeq Tp, const PackedSeq Pp) {
  const CmpCtx cx{T, Tp, n, pats, Pp};
  const unsigned long long base = pat_off[blockIdx.x];
  const uint32_t m = (uint32_t)(pat_off[blockIdx.x + 1] - base);
  const uint8_t* P = pats + base;
  for (uint32_t i = threadIdx.x; i < m; i += 64) {
    const uint32_t thr = thr_in[base + i];
    uint32_t c = 0;
    if (thr != NONE) {
      const uint32_t lo = lo_in[base + i], hi = hi_in[base + i];
      for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t t = sa[k];
        if (prev_excluded(T, t, P, i)) continue;
        const uint32_t l = extend(cx, t, base, m, i, prm.L);
        if (l < thr) continue;
        c += t == 0 ? zero_copies(cx, base, sa, key, sigma, P, m, i, prm.L, lo, hi, l) : 1u;
      }
    }
    cnt_out[base + i] = c;
  }
}

struct Cand { uint32_t t, l; };

// write the candidates of each position, sort them by t, apply filter (a)
// (src/max-emb-graph.c:301-334) and move the survivors to the front of the position's slot
__global__ __launch_bounds__(64)
void pair_fill_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint32_t* __restrict__ sa,
                      const uint8_t* __restrict__ key, uint32_t sigma,
                      const uint8_t* __restrict__ pats, const unsigned long long* __restrict__ pat_off,
                      PairParams prm, const uint32_t* __restrict__ lo_in, const uint32_t* __restrict__ hi_in,
                      const uint32_t* __restrict__ thr_in, const unsigned long long* __restrict__ cand_off,
                      Cand* __restrict__ cand, uint32_t* __restrict__ cnt_a, const PackedSeq Tp, const PackedSeq Pp) {
  const CmpCtx cx{T, Tp, n, pats, Pp};
  const unsigned long long base = pat_off[blockIdx.x];
  const uint32_t m = (uint32_t)(pat_off[blockIdx.x + 1] - base);
  const uint8_t* P = pats + base;
  for (uint32_t i = threadIdx.x; i < m; i += 64) {
    const uint32_t thr = thr_in[base + i];
    uint32_t c = 0;
    if (thr != NONE) {
      Cand* slot = cand + cand_off[base + i];
      const uint32_t lo = lo_in[base + i], hi = hi_in[base + i];
      for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t t = sa[k];
        if (prev_excluded(T, t, P, i)) continue;
        const uint32_t l = extend(cx, t, base, m, i, prm.L);
        if (l < thr) continue;
        // insertion sort by t (distinct, except the copies of t == 0, which stay together in front)
        const uint32_t copies = t == 0 ? zero_copies(cx, base, sa, key, sigma, P, m, i, prm.L, lo, hi, l) : 1u;
        for (uint32_t cpy = 0; cpy < copies; ++cpy) {
          uint32_t q = c++;
          while (q > 0 && slot[q - 1].t > t) { slot[q] = slot[q - 1]; --q; }
          slot[q].t = t; slot[q].l = l;
        }
      }
      // filter (a): PJ dies when an earlier PI (smaller t) covers it or is its twin shifted by one.
      // The reference tests against ALL earlier entries, dead ones included, so deaths are
      // decided on the unmodified sorted list: mark with the top bit of l, then compact.
      for (uint32_t j = c; j-- > 1;) {
        const uint32_t tj = slot[j].t, lj = slot[j].l & 0x7FFFFFFFu;
        for (uint32_t q = j; q-- > 0;) {
          const uint32_t ti = slot[q].t, li = slot[q].l & 0x7FFFFFFFu;
          if ((tj > ti && tj + lj <= ti + li) || (tj == ti + 1 && lj == li)) { slot[j].l |= 0x80000000u; break; }
        }
      }
      uint32_t w = 0;
      for (uint32_t k = 0; k < c; ++k)
        if (!(slot[k].l & 0x80000000u)) slot[w++] = slot[k];
      c = w;
    }
    cnt_a[base + i] = c;
  }
}

// filter (b) (src/max-emb-graph.c:349-375): position i loses I1 when position i-1 (after filter
// (a), before (b)) holds I with I.t == I1.t and I.l >= I1.l.  Flags only: lists stay intact.
__global__ __launch_bounds__(64)
void pair_cross_kernel(const unsigned long long* __restrict__ pat_off,
                       const unsigned long long* __restrict__ cand_off, const Cand* __restrict__ cand,
                       const uint32_t* __restrict__ cnt_a, uint8_t* __restrict__ keep,
                       uint32_t* __restrict__ cnt_b) {
  const unsigned long long base = pat_off[blockIdx.x];
  const uint32_t m = (uint32_t)(pat_off[blockIdx.x + 1] - base);
  for (uint32_t i = threadIdx.x; i < m; i += 64) {
    const uint32_t c = cnt_a[base + i];
    const unsigned long long off = cand_off[base + i];
    uint32_t kept = 0;
    if (c) {
      const uint32_t cp = i > 0 ? cnt_a[base + i - 1] : 0;
      const Cand* prev = i > 0 ? cand + cand_off[base + i - 1] : nullptr;
      for (uint32_t k = 0; k < c; ++k) {
        const Cand x = cand[off + k];
        bool rim = false;
        for (uint32_t q = 0; q < cp && !rim; ++q) rim = prev[q].t == x.t && prev[q].l >= x.l;
        keep[off + k] = rim ? 0 : 1;
        kept += rim ? 0 : 1;
      }
    }
    cnt_b[base + i] = kept;
  }
}

__global__ __launch_bounds__(64)
void pair_emit_kernel(const unsigned long long* __restrict__ pat_off,
                      const unsigned long long* __restrict__ cand_off, const Cand* __restrict__ cand,
                      const uint32_t* __restrict__ cnt_a, const uint8_t* __restrict__ keep,
                      const unsigned long long* __restrict__ out_off, pgpu_pairing* __restrict__ out,
                      unsigned long long* __restrict__ out_first, uint32_t n_pat, unsigned long long total_pos) {
  const unsigned long long base = pat_off[blockIdx.x];
  const uint32_t m = (uint32_t)(pat_off[blockIdx.x + 1] - base);
  if (threadIdx.x == 0) {
    out_first[blockIdx.x] = base < total_pos ? out_off[base] : out_off[total_pos];
    if (blockIdx.x == n_pat - 1) out_first[n_pat] = out_off[total_pos];
  }
  for (uint32_t i = threadIdx.x; i < m; i += 64) {
    const uint32_t c = cnt_a[base + i];
    const unsigned long long off = cand_off[base + i];
    unsigned long long w = out_off[base + i];
    for (uint32_t k = 0; k < c; ++k) {
      if (!keep[off + k]) continue;
      out[w].p = (int32_t)i; out[w].t = (int32_t)cand[off + k].t; out[w].l = (int32_t)cand[off + k].l;
      ++w;
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C-ABI: the plan (create = patterns resident in HBM; run* = the kernels of a stage; fetch* = its results)
// ---------------------------------------------------------------------------------------------
// Which results a plan holds.  Every stage reads what the stage before it left in HBM, so this is one value.  The rule:
// a run of stage k first lowers the plan to k - 1 -- its own results and everything made from them are gone, even when
// the call is then refused --, asks for stage k - 1 (made with the same min_factor_len, where run_meg and run_candidates
// compare one), and raises the plan to k when it succeeds.  A fetch of stage k asks for stage k.  A plan without
// patterns has nothing to compute: its runs succeed without their predecessor (run_factorizations and the stages above
// it still ask for theirs), and fetch and fetch_meg answer whatever ran.
// The candidate lists (run_candidate_lists, pgpu_enum.hip) are a branch beside this ladder, not a rung: the run asks for
// RECORDS made with the same min_factor_len and never changes `stage`; its results live in pool slots of their own
// (SLOT_ENUM, SLOT_ENUM_OUT) under a flag of their own (lists_valid), which run and run_meg clear and which the run of
// another resident plan overrules (overwritten); run_candidates and the rungs above it neither need nor disturb them.
// The factorization lists (run_factorization_lists, pgpu_flists.hip) are a second branch, built the same way: the run asks
// for valid candidate lists and reads them where they lie; its results live in SLOT_FLIST (the workspace in SLOT_FLIST_WS)
// under flists_valid, which run, run_meg and run_candidate_lists clear; it needs and disturbs no rung.
enum Stage : int { NOTHING, PAIRINGS, RECORDS, CANDIDATES, FACTORIZATIONS, FINALS, UNITS, TEXTS, SIDES };

// the plan's events (made only when the context times its calls): seven around the six pairing stages, a pair each for
// the MEG and the candidate stage, the eight of pgpu_fact_job, the six of pgpu_final_job, the pair of pgpu_unit_job, the
// three of pgpu_text_job, the three of pgpu_side_job, the pair of the candidate lists, the ten of pgpu_flist_job
enum { EV_PAIRS = 0, EV_MEG = 7, EV_CAND = 9, EV_FACT = 11, EV_FINAL = 19, EV_UNITS = 25, EV_TEXTS = 27, EV_SIDES = 30, EV_LISTS = 33, EV_FLISTS = 35, N_EVENTS = 45 };

struct pgpu_pairing_plan {
  pgpu_ctx* owner = nullptr;
  const pgpu_index* idx = nullptr;                     // for the views the small stage takes (pgpu_index_lcf_view, pgpu_class_view_get)
  PairIndexView ix{};
  size_t n_pat = 0;
  unsigned long long total_pos = 0;
  Stage stage = NOTHING;
  uint32_t last_L = 0, meg_L = 0;                      // min_factor_len of the last run, of the last run_meg
  bool pooled = false;
  // resident plan: only the patterns (bytes, offsets, packed) are the plan's own -- one allocation -- and every
  // buffer a run writes comes from the context's pool, shared with the other resident plans of the context
  bool resident = false;
  void* d_resident = nullptr;
  uint8_t* d_pats = nullptr;
  unsigned long long* d_pat_off = nullptr;
  uint32_t *d_pcode = nullptr, *d_pbad = nullptr;     // the patterns at 2 bits per base + flag bits (PackedSeq)
  // the original sequences of the patterns that have one, behind the pattern bytes in d_pats: one offset per pattern
  // (d_pat_off itself in a plan without originals), and the bytes that lie behind d_pats in all
  unsigned long long* d_orig_off = nullptr;
  size_t seq_bytes = 0;
  hipEvent_t ev[N_EVENTS] = {nullptr};
  // pairings
  uint32_t *d_lo = nullptr, *d_hi = nullptr, *d_a = nullptr, *d_thr = nullptr, *d_cnt = nullptr,
           *d_cnt_a = nullptr, *d_cnt_b = nullptr;
  unsigned long long *d_cand_off = nullptr, *d_out_off = nullptr, *d_out_first = nullptr;
  void* d_tmp = nullptr;                               // of the exclusive scans of every stage
  size_t tmp_bytes = 0;
  Cand* d_cand = nullptr;
  uint8_t* d_keep = nullptr;
  pgpu_pairing* d_out = nullptr;
  size_t cand_cap = 0, keep_cap = 0, out_cap = 0;
  unsigned long long n_cand = 0, n_out = 0;
  float ms[6] = {0};
  // MEG stage (pgpu_meg.hip)
  void *d_meg_scratch = nullptr, *d_meg_info = nullptr;
  uint32_t* d_meg_bytes = nullptr;
  unsigned long long* d_meg_off = nullptr;
  uint8_t* d_meg_out = nullptr;
  size_t meg_cap = 0;
  unsigned long long meg_total = 0;
  float meg_ms = 0.f;
  // candidate stage (pgpu_cand.hip) over the records of the last run_meg
  pgpu_cand_result* d_cand_res = nullptr;
  uint32_t* d_cand_cnt = nullptr;
  unsigned long long* d_cand_first = nullptr;
  pgpu_factor* d_cand_exons = nullptr;
  size_t cand_exons_cap = 0;
  unsigned long long cand_total = 0;
  float cand_ms = 0.f;
  // factorization stage (pgpu_fact.hip) over the candidates of the last run_candidates
  uint8_t *d_fact = nullptr, *d_fact_ws = nullptr;      // the driver's block; the workspace of clean and refine
  size_t fact_cap = 0, fact_ws_cap = 0;
  unsigned long long fact_total = 0;
  float fact_ms[4] = {0};
  // final stage (pgpu_final.hip) over the factorizations of the last run_factorizations
  uint8_t* d_final = nullptr;
  size_t final_cap = 0;
  unsigned long long final_total = 0;
  float final_ms[3] = {0};
  // unit stage (pgpu_unit.hip) over the finals of the last run_final_factorizations and the headers of the records
  uint8_t* d_unit = nullptr;
  size_t unit_cap = 0, n_units = 0;
  unsigned long long unit_total = 0;
  float unit_ms = 0.f;
  // text stage (pgpu_text.hip) over the units of the last run_units: the stage's block, and the two blobs (raw, then pests
  // at text_pests_at), which are sized after the count pass
  uint8_t *d_text = nullptr, *d_text_blobs = nullptr;
  size_t text_cap = 0, text_blobs_cap = 0, text_pests_at = 0, text_headers_len = 0;
  unsigned long long text_raw_total = 0, text_pests_total = 0;
  bool text_timed = false;                             // the write pass's event is still to be waited for
  float text_ms = 0.f, text_write_ms = 0.f;
  // side stage (pgpu_side.hip) over the records of the last run_meg, the units of the last run_units and the headers of the
  // last run_texts: the stage's block, and the three blobs in one allocation (side_blobs), sized after the count pass
  uint8_t *d_side = nullptr, *d_side_blobs = nullptr;
  size_t side_cap = 0, side_blobs_cap = 0;
  unsigned long long side_total[3] = {0, 0, 0};
  bool side_timed = false;                             // the write pass's event is still to be waited for
  float side_ms = 0.f, side_write_ms = 0.f;
  // candidate lists (pgpu_enum.hip) over the records of the last run_meg, beside the ladder: the block of enum_layout
  // (pgpu_enum.h; results, counts, offsets) and the one of enum_out_layout (candidate table, exons), sized after the scans
  uint8_t *d_lists = nullptr, *d_lists_out = nullptr;
  size_t lists_cap = 0, lists_out_cap = 0;
  unsigned long long lists_cands = 0, lists_exons = 0;
  bool lists_valid = false;
  float lists_ms = 0.f;
  // factorization lists (pgpu_flists.hip) over those candidate lists, beside the ladder too: the driver's block
  // (flist_layout of pgpu_flists.h, for the counts the lists had at the run) and the workspace of clean and refine
  uint8_t *d_flist = nullptr, *d_flist_ws = nullptr;
  size_t flist_cap = 0, flist_ws_cap = 0;
  unsigned long long flist_cands = 0, flist_cand_exons = 0, flist_facts = 0, flist_exons = 0;
  bool flists_valid = false;
  float flist_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
};

static void lower(pgpu_pairing_plan* p, Stage s) { if (p->stage > s) p->stage = s; }
static int reached(pgpu_pairing_plan* p, Stage s) { p->stage = s; return PGPU_OK; }

// inside an entry whose context is named `ctx`: a failing HIP call, or a buffer that could not be had, ends the entry
#define PLAN_TRY(call)                                                                          \
  do {                                                                                          \
    const hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) return pgpu_ctx_fail(ctx, pgpu_code_of(e_), hipGetErrorString(e_));   \
  } while (0)
#define PLAN_NEED(ptr) do { if (!(ptr)) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of device memory (pairing plan)"); } while (0)

// device buffer for a pairing plan: from the context's pool when the plan holds it
template <class T> static T* plan_alloc(pgpu_pairing_plan* p, PlanSlot slot, size_t count) {
  const size_t bytes = (count ? count : 1) * sizeof(T);
  if (p->pooled) return (T*)pgpu_ctx_pool_get(p->owner, PLAN_POOL, slot, bytes);
  void* q = nullptr;
  if (hipMalloc(&q, bytes) != hipSuccess) return nullptr;
  pgpu_trace_alloc("plan device", q, bytes);
  return (T*)q;
}

// A buffer whose size is known only once a stage has counted: `ptr` when it is there and holds `need` elements, otherwise a
// new one of need + slack in its place (*cap follows).  Null when there is no memory.
template <class T> static T* plan_grow(pgpu_pairing_plan* p, T* ptr, size_t* cap, size_t need, size_t slack, PlanSlot slot) {
  if (ptr && need <= *cap) return ptr;
  if (!p->pooled) (void)hipFree(ptr);
  ptr = plan_alloc<T>(p, slot, need + slack);
  *cap = ptr ? need + slack : 0;
  return ptr;
}

// The eleven buffers a run writes from its first kernel on.  An ordinary plan takes them once; a resident one takes them
// from the shared pool anew at every run (another plan may have made the pool grow, i.e. move, in between).
static bool run_buffers(pgpu_pairing_plan* p) {
  const size_t tp = (size_t)p->total_pos, n_pat = p->n_pat;
  p->d_lo = plan_alloc<uint32_t>(p, SLOT_LO, tp); p->d_hi = plan_alloc<uint32_t>(p, SLOT_HI, tp);
  p->d_a = plan_alloc<uint32_t>(p, SLOT_A, tp); p->d_thr = plan_alloc<uint32_t>(p, SLOT_THR, tp);
  p->d_cnt = plan_alloc<uint32_t>(p, SLOT_CNT, tp + 1); p->d_cnt_a = plan_alloc<uint32_t>(p, SLOT_CNT_A, tp + 1);
  p->d_cnt_b = plan_alloc<uint32_t>(p, SLOT_CNT_B, tp + 1);
  p->d_cand_off = plan_alloc<unsigned long long>(p, SLOT_CAND_OFF, tp + 1);
  p->d_out_off = plan_alloc<unsigned long long>(p, SLOT_OUT_OFF, tp + 1);
  p->d_out_first = plan_alloc<unsigned long long>(p, SLOT_OUT_FIRST, n_pat + 1);
  p->d_tmp = plan_alloc<uint8_t>(p, SLOT_TMP, p->tmp_bytes);
  return p->d_lo && p->d_hi && p->d_a && p->d_thr && p->d_cnt && p->d_cnt_a && p->d_cnt_b && p->d_cand_off && p->d_out_off &&
         p->d_out_first && p->d_tmp;
}

// a resident plan whose shared buffers the run of another resident plan has written since: nothing of its results is left
static bool overwritten(pgpu_ctx* ctx, const pgpu_pairing_plan* p) {
  return p->resident && p->n_pat && pgpu_ctx_pool_owner(ctx, PLAN_POOL) != p;
}
// PGPU_OK, or the refusal of such a plan, which no longer holds `what`
static int still_owns(pgpu_ctx* ctx, const pgpu_pairing_plan* p, const char* what) {
  if (!overwritten(ctx, p)) return PGPU_OK;
  char msg[96];
  snprintf(msg, sizeof msg, "the %s of this resident plan were overwritten by the run of another one", what);
  return pgpu_ctx_fail(ctx, PGPU_EINVAL, msg);
}
// fetch and fetch_meg ask for their stage first -- on a plan with patterns; one without answers whatever ran -- but leave
// an overwritten plan to the refusal above, whatever its rung: that is the answer callers of these two entries know
static bool missing(pgpu_ctx* ctx, const pgpu_pairing_plan* p, Stage s) { return p->n_pat && p->stage < s && !overwritten(ctx, p); }

// `count` events from ev[first] on, once, when the context times its calls
static hipError_t plan_events(pgpu_pairing_plan* p, int first, int count) {
  if (!pgpu_ctx_timing(p->owner) || p->ev[first]) return hipSuccess;
  for (int k = first; k < first + count; ++k) {
    const hipError_t e = hipEventCreate(&p->ev[k]);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// A count pass has written counts[0..n): drive_scan into offsets, and *total = offsets[n] on the host, waited for.  `ev` (may
// be null) is recorded behind the scan, where the pairing stages end their count+scan time.
static hipError_t scan_total(pgpu_ctx* ctx, const pgpu_pairing_plan* p, uint32_t* counts, unsigned long long* offsets, size_t n,
                             hipEvent_t ev, unsigned long long* total) {
  hipStream_t st = pgpu_ctx_stream(ctx);
  DRIVE(drive_scan(counts, offsets, n, p->d_tmp, st));
  if (ev) DRIVE(hipEventRecord(ev, st));
  DRIVE(hipMemcpyAsync(total, offsets + n, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  return pgpu_ctx_wait(ctx);
}

// the one block of a rung from four to eight, with an eighth to spare; a resident plan takes it anew: the pool may have moved
static uint8_t* stage_block(pgpu_pairing_plan* p, uint8_t* ptr, size_t* cap, size_t total, PlanSlot slot) {
  return plan_grow(p, p->resident ? nullptr : ptr, cap, total, total / 8, slot);
}
// after the wait: the times between `pairs` pairs of events from ev[first] on, when the plan has them
static void elapsed_pairs(const pgpu_pairing_plan* p, int first, int pairs, float* ms) {
  if (p->ev[first]) for (int k = 0; k < pairs; ++k) hipEventElapsedTime(&ms[k], p->ev[first + 2 * k], p->ev[first + 2 * k + 1]);
}

static void pairing_plan_free(pgpu_pairing_plan* p) {
  if (!p) return;
  if (p->resident) { pgpu_ctx_pool_unshare(p->owner, PLAN_POOL, p); hipFree(p->d_resident); }
  else if (p->pooled) pgpu_ctx_pool_release(p->owner, PLAN_POOL);
  else {
    hipFree(p->d_pats); hipFree(p->d_pcode); hipFree(p->d_pbad); hipFree(p->d_pat_off); hipFree(p->d_lo); hipFree(p->d_hi); hipFree(p->d_a);
    hipFree(p->d_thr); hipFree(p->d_cnt); hipFree(p->d_cnt_a); hipFree(p->d_cnt_b);
    hipFree(p->d_cand_off); hipFree(p->d_out_off); hipFree(p->d_out_first); hipFree(p->d_cand);
    hipFree(p->d_keep); hipFree(p->d_out); hipFree(p->d_tmp);
    hipFree(p->d_meg_scratch); hipFree(p->d_meg_info); hipFree(p->d_meg_bytes); hipFree(p->d_meg_off); hipFree(p->d_meg_out);
    hipFree(p->d_cand_res); hipFree(p->d_cand_cnt); hipFree(p->d_cand_first); hipFree(p->d_cand_exons);
    hipFree(p->d_fact); hipFree(p->d_fact_ws); hipFree(p->d_final); hipFree(p->d_unit); hipFree(p->d_text); hipFree(p->d_text_blobs);
    hipFree(p->d_side); hipFree(p->d_side_blobs); hipFree(p->d_lists); hipFree(p->d_lists_out);
    hipFree(p->d_flist); hipFree(p->d_flist_ws);
    if (p->d_orig_off != p->d_pat_off) hipFree(p->d_orig_off);
  }
  for (auto& e : p->ev) if (e) hipEventDestroy(e);
  delete p;
}

static int pairing_plan_create(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns,
                               const uint64_t* pat_off, size_t n_pat, bool resident, const uint32_t* orig_pat,
                               const uint64_t* orig_first, const char* orig_bytes, size_t n_orig, pgpu_pairing_plan** out) {
  if (!ctx || !idx || !out || !pat_off || (n_pat && pat_off[n_pat] && !patterns)) return PGPU_EINVAL;
  *out = nullptr;
  for (size_t i = 0; i < n_pat; ++i)
    if (pat_off[i + 1] < pat_off[i] || pat_off[i + 1] - pat_off[i] > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad pattern offsets");
  if (const char* wrong = originals_wrong(pat_off, n_pat, orig_pat, orig_first, orig_bytes, n_orig)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  const size_t orig_total = n_orig ? (size_t)(orig_first[n_orig] - orig_first[0]) : 0;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  std::unique_ptr<pgpu_pairing_plan, void (*)(pgpu_pairing_plan*)> hold(new (std::nothrow) pgpu_pairing_plan(), pairing_plan_free);
  pgpu_pairing_plan* p = hold.get();
  if (!p) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of host memory");
  hipStream_t st = pgpu_ctx_stream(ctx);
  p->owner = ctx; p->idx = idx; p->ix = pgpu_index_pair_view(idx);
  p->n_pat = n_pat; p->total_pos = n_pat ? pat_off[n_pat] : 0;
  const size_t tp = (size_t)p->total_pos, bad_words = (tp + 31) / 32;
  p->resident = resident && pgpu_ctx_pool_share(ctx, PLAN_POOL);
  p->pooled = p->resident || pgpu_ctx_pool_acquire(ctx, PLAN_POOL);
  p->tmp_bytes = pgpu_scan_tmp_bytes(std::max(tp, n_pat) + 1);
  if (p->resident) {
    const size_t o_off = up256(tp + orig_total + 64), o_code = o_off + up256((n_pat + 1) * sizeof(unsigned long long)),
                 o_bad = o_code + up256((2 * bad_words + 4) * sizeof(uint32_t)), o_orig = o_bad + up256((bad_words + 4) * sizeof(uint32_t)),
                 total = o_orig + (n_orig ? up256(n_pat * sizeof(unsigned long long)) : 0);
    PLAN_TRY(hipMalloc(&p->d_resident, total));
    pgpu_trace_alloc("resident plan", p->d_resident, total);
    uint8_t* base = (uint8_t*)p->d_resident;
    p->d_pats = base; p->d_pat_off = (unsigned long long*)(base + o_off);
    p->d_pcode = (uint32_t*)(base + o_code); p->d_pbad = (uint32_t*)(base + o_bad);
    p->d_orig_off = n_orig ? (unsigned long long*)(base + o_orig) : p->d_pat_off;
  } else {
    PLAN_NEED(p->d_pats = plan_alloc<uint8_t>(p, SLOT_PATS, tp + orig_total + 64));
    PLAN_NEED(p->d_pat_off = plan_alloc<unsigned long long>(p, SLOT_PAT_OFF, n_pat + 1));
    p->d_orig_off = p->d_pat_off;
    if (n_orig) PLAN_NEED(p->d_orig_off = plan_alloc<unsigned long long>(p, SLOT_ORIG_OFF, n_pat));
    PLAN_NEED(run_buffers(p));
    PLAN_NEED(p->d_pcode = plan_alloc<uint32_t>(p, SLOT_PCODE, 2 * bad_words + 4));
    PLAN_NEED(p->d_pbad = plan_alloc<uint32_t>(p, SLOT_PBAD, bad_words + 4));
  }
  PLAN_TRY(plan_events(p, EV_PAIRS, EV_MEG - EV_PAIRS));
  if (tp) PLAN_TRY(hipMemcpyAsync(p->d_pats, patterns, tp, hipMemcpyHostToDevice, st));
  PLAN_TRY(hipMemcpyAsync(p->d_pat_off, pat_off, (n_pat + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  p->seq_bytes = tp + orig_total;
  std::unique_ptr<unsigned long long[]> table;         // alive until the copy has been waited for
  if (n_orig) {
    // the table of original offsets: a pattern's own offset, or where its original lies behind the patterns
    table.reset(new (std::nothrow) unsigned long long[n_pat]);
    if (!table) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of host memory");
    for (size_t i = 0; i < n_pat; ++i) table[i] = pat_off[i];
    for (size_t k = 0; k < n_orig; ++k) table[orig_pat[k]] = tp + (orig_first[k] - orig_first[0]);
    PLAN_TRY(hipMemcpyAsync(p->d_orig_off, table.get(), n_pat * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    if (orig_total) PLAN_TRY(hipMemcpyAsync(p->d_pats + tp, orig_bytes + orig_first[0], orig_total, hipMemcpyHostToDevice, st));
  }
  PLAN_TRY(pack_sequence(p->d_pats, tp, p->d_pcode, p->d_pbad, st));
  PLAN_TRY(hipStreamSynchronize(st));
  *out = hold.release();
  return PGPU_OK;
}

extern "C" int pgpu_pairing_plan_create(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns,
                                        const uint64_t* pat_off, size_t n_pat, pgpu_pairing_plan** out) {
  return pairing_plan_create(ctx, idx, patterns, pat_off, n_pat, false, nullptr, nullptr, nullptr, 0, out);
}
extern "C" int pgpu_pairing_plan_create_resident(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns,
                                                 const uint64_t* pat_off, size_t n_pat, pgpu_pairing_plan** out) {
  return pairing_plan_create(ctx, idx, patterns, pat_off, n_pat, true, nullptr, nullptr, nullptr, 0, out);
}
extern "C" int pgpu_pairing_plan_create_with_originals(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns,
                                                       const uint64_t* pat_off, size_t n_pat, int resident, const uint32_t* orig_pat,
                                                       const uint64_t* orig_first, const char* orig_bytes, size_t n_orig,
                                                       pgpu_pairing_plan** out) {
  return pairing_plan_create(ctx, idx, patterns, pat_off, n_pat, resident != 0, orig_pat, orig_first, orig_bytes, n_orig, out);
}

extern "C" int pgpu_pairing_plan_destroy(pgpu_ctx* ctx, pgpu_pairing_plan* p) {
  if (!ctx || !p) return PGPU_EINVAL;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStreamSynchronize(pgpu_ctx_stream(ctx));
  pairing_plan_free(p);
  return PGPU_OK;
}

// ---- pairings ---------------------------------------------------------------------------------------------------
// runs every kernel; the size-dependent buffers (candidates, output) grow on demand, which costs one wait after
// each scan (the totals are needed on the host anyway)
extern "C" int pgpu_pairing_plan_run(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_pairing_params* params) {
  if (!ctx || !p || !params || params->min_factor_len == 0) return PGPU_EINVAL;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  p->n_cand = p->n_out = 0;
  lower(p, NOTHING);
  p->lists_valid = p->flists_valid = false;
  p->last_L = params->min_factor_len;
  if (p->n_pat == 0) return reached(p, PAIRINGS);
  if (p->resident) {
    pgpu_ctx_pool_set_owner(ctx, PLAN_POOL, p);       // whatever another resident plan left there is gone from here on
    p->d_cand = nullptr; p->d_keep = nullptr; p->d_out = nullptr;              // sized (and taken) once the counts are known
    p->d_meg_scratch = nullptr; p->d_meg_out = nullptr;
    PLAN_NEED(run_buffers(p));
  }
  hipStream_t st = pgpu_ctx_stream(ctx);
  const PairIndexView& ix = p->ix;
  const size_t tp = (size_t)p->total_pos;
  const PairParams prm{params->min_factor_len, params->min_string_depth_rate};
  const PackedSeq Tp{ix.code, ix.bad}, Pp{p->d_pcode, p->d_pbad};
  const dim3 pgrid((unsigned)p->n_pat), pblk(64);
  const ProfRange range("pairings");
  PLAN_TRY(drive_record(p->ev, 0, st));
  hipLaunchKernelGGL(pair_locate_kernel, pgrid, pblk, 0, st, ix.T, ix.n, ix.sa, ix.klo, ix.khi, p->d_pats, p->d_pat_off, prm, p->d_lo, p->d_hi, p->d_a, Tp, Pp);
  PLAN_TRY(drive_record(p->ev, 1, st));
  hipLaunchKernelGGL(pair_chain_kernel, dim3((unsigned)((p->n_pat + 63) / 64)), pblk, 0, st, ix.T, ix.n, ix.sa, ix.lcp,
                     p->d_pats, p->d_pat_off, (uint32_t)p->n_pat, prm, p->d_lo, p->d_hi, p->d_a, p->d_thr, Tp, Pp);
  PLAN_TRY(drive_record(p->ev, 2, st));
  hipLaunchKernelGGL(pair_count_kernel, pgrid, pblk, 0, st, ix.T, ix.n, ix.sa, ix.key, ix.sigma, p->d_pats, p->d_pat_off, prm, p->d_lo, p->d_hi, p->d_thr, p->d_cnt, Tp, Pp);
  PLAN_TRY(scan_total(ctx, p, p->d_cnt, p->d_cand_off, tp, p->ev[3], &p->n_cand));
  PLAN_NEED(p->d_cand = plan_grow(p, p->d_cand, &p->cand_cap, (size_t)p->n_cand, (size_t)p->n_cand / 8 + 1024, SLOT_CAND));
  PLAN_NEED(p->d_keep = plan_grow(p, p->d_keep, &p->keep_cap, (size_t)p->n_cand, (size_t)p->n_cand / 8 + 1024, SLOT_KEEP));
  hipLaunchKernelGGL(pair_fill_kernel, pgrid, pblk, 0, st, ix.T, ix.n, ix.sa, ix.key, ix.sigma, p->d_pats, p->d_pat_off, prm, p->d_lo, p->d_hi, p->d_thr,
                     p->d_cand_off, p->d_cand, p->d_cnt_a, Tp, Pp);
  PLAN_TRY(drive_record(p->ev, 4, st));
  hipLaunchKernelGGL(pair_cross_kernel, pgrid, pblk, 0, st, p->d_pat_off, p->d_cand_off, p->d_cand, p->d_cnt_a, p->d_keep, p->d_cnt_b);
  PLAN_TRY(scan_total(ctx, p, p->d_cnt_b, p->d_out_off, tp, p->ev[5], &p->n_out));
  PLAN_NEED(p->d_out = plan_grow(p, p->d_out, &p->out_cap, (size_t)p->n_out, (size_t)p->n_out / 8 + 1024, SLOT_OUT));
  hipLaunchKernelGGL(pair_emit_kernel, pgrid, pblk, 0, st, p->d_pat_off, p->d_cand_off, p->d_cand, p->d_cnt_a, p->d_keep, p->d_out_off,
                     p->d_out, p->d_out_first, (uint32_t)p->n_pat, p->total_pos);
  PLAN_TRY(drive_record(p->ev, 6, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  PLAN_TRY(hipGetLastError());
  if (p->ev[0]) for (int k = 0; k < 6; ++k) hipEventElapsedTime(&p->ms[k], p->ev[k], p->ev[k + 1]);
  return reached(p, PAIRINGS);
}

extern "C" uint64_t pgpu_pairing_plan_count(const pgpu_pairing_plan* p) { return p ? p->n_out : 0; }
extern "C" uint64_t pgpu_pairing_plan_positions(const pgpu_pairing_plan* p) { return p ? p->total_pos : 0; }
extern "C" double pgpu_pairing_plan_kernel_ms(const pgpu_pairing_plan* p, int k) { return (p && k >= 0 && k < 6) ? p->ms[k] : 0.0; }

extern "C" int pgpu_pairing_plan_fetch(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_pairing* out, size_t out_cap,
                                       uint64_t* out_first) {
  if (!ctx || !p || !out_first) return PGPU_EINVAL;
  if (missing(ctx, p, PAIRINGS)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch needs pgpu_pairing_plan_run first");
  if (out_cap < p->n_out) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "pairing buffer too small");
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0) { out_first[0] = 0; return PGPU_OK; }
  if (p->n_out) PLAN_TRY(hipMemcpyAsync(out, p->d_out, (size_t)p->n_out * sizeof(pgpu_pairing), hipMemcpyDeviceToHost, st));
  PLAN_TRY(hipMemcpyAsync(out_first, p->d_out_first, (p->n_pat + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- MEG of every pattern from the pairings that pgpu_pairing_plan_run left in HBM --------------------------------
extern "C" int pgpu_pairing_plan_run_meg(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_meg_params* prm) {
  if (!ctx || !p || !prm || prm->min_factor_len == 0) return PGPU_EINVAL;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  p->meg_total = 0; p->meg_ms = 0.f;
  lower(p, PAIRINGS);
  p->lists_valid = p->flists_valid = false;
  if (p->n_pat == 0) return reached(p, RECORDS);
  if (p->stage < PAIRINGS || p->last_L != prm->min_factor_len)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_meg needs the pairings of pgpu_pairing_plan_run with the same min_factor_len");
  if (const int rc = still_owns(ctx, p, "pairings")) return rc;
  if (p->resident) { p->d_meg_scratch = nullptr; p->d_meg_out = nullptr; }
  hipStream_t st = pgpu_ctx_stream(ctx);
  const uint32_t np = (uint32_t)p->n_pat;
  const ProfRange range("meg");
  if (!p->d_meg_scratch) {
    PLAN_NEED(p->d_meg_scratch = plan_alloc<uint8_t>(p, SLOT_MEG_SCRATCH, pgpu_meg_scratch_bytes(np)));
    PLAN_NEED(p->d_meg_info = plan_alloc<uint8_t>(p, SLOT_MEG_INFO, (size_t)np * 16));
    PLAN_NEED(p->d_meg_bytes = plan_alloc<uint32_t>(p, SLOT_MEG_BYTES, (size_t)np + 1));
    PLAN_NEED(p->d_meg_off = plan_alloc<unsigned long long>(p, SLOT_MEG_OFF, (size_t)np + 1));
    PLAN_TRY(plan_events(p, EV_MEG, 2));
  }
  PLAN_TRY(drive_record(p->ev, EV_MEG, st));
  pgpu_meg_launch_build(p->d_out, p->d_out_first, p->d_pat_off, np, prm, p->d_meg_scratch, p->d_meg_info, p->d_meg_bytes, st);
  PLAN_TRY(scan_total(ctx, p, p->d_meg_bytes, p->d_meg_off, np, nullptr, &p->meg_total));
  PLAN_NEED(p->d_meg_out = plan_grow(p, p->d_meg_out, &p->meg_cap, (size_t)p->meg_total, (size_t)p->meg_total / 8 + 4096, SLOT_MEG_OUT));
  pgpu_meg_launch_emit(np, p->d_meg_scratch, p->d_meg_info, p->d_meg_off, p->d_meg_out, st);
  PLAN_TRY(drive_record(p->ev, EV_MEG + 1, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  PLAN_TRY(hipGetLastError());
  elapsed_pairs(p, EV_MEG, 1, &p->meg_ms);
  p->meg_L = prm->min_factor_len;
  return reached(p, RECORDS);
}

extern "C" uint64_t pgpu_pairing_plan_meg_bytes(const pgpu_pairing_plan* p) { return p ? p->meg_total : 0; }
extern "C" double pgpu_pairing_plan_meg_ms(const pgpu_pairing_plan* p) { return p ? p->meg_ms : 0.0; }

extern "C" int pgpu_pairing_plan_fetch_meg(pgpu_ctx* ctx, pgpu_pairing_plan* p, void* out, size_t out_cap, uint64_t* rec_first) {
  if (!ctx || !p || !rec_first || (p->meg_total && !out)) return PGPU_EINVAL;
  if (missing(ctx, p, RECORDS)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_meg needs pgpu_pairing_plan_run_meg first");
  if (out_cap < p->meg_total) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "MEG buffer too small");
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0) { rec_first[0] = 0; return PGPU_OK; }
  if (p->meg_total) PLAN_TRY(hipMemcpyAsync(out, p->d_meg_out, (size_t)p->meg_total, hipMemcpyDeviceToHost, st));
  PLAN_TRY(hipMemcpyAsync(rec_first, p->d_meg_off, (p->n_pat + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- the candidate factorization of every record that pgpu_pairing_plan_run_meg left in HBM (pgpu_cand.hip) -------
extern "C" int pgpu_pairing_plan_run_candidates(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_cand_params* prm) {
  if (!ctx || !p || !prm) return PGPU_EINVAL;
  p->cand_total = 0; p->cand_ms = 0.f;                 // cand_total stays 0 unless the run succeeds
  lower(p, RECORDS);
  if (prm->min_factor_len == 0 || prm->min_factor_len > (1u << 24))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad candidate parameters (min_factor_len 0 or above 2^24)");
  if (p->n_pat == 0) return reached(p, CANDIDATES);
  if (p->stage < RECORDS || p->meg_L != prm->min_factor_len)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_candidates needs the records of pgpu_pairing_plan_run_meg with the same min_factor_len");
  if (const int rc = still_owns(ctx, p, "records")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  if (p->resident) { p->d_cand_res = nullptr; p->d_cand_exons = nullptr; }     // taken anew: the pool may have moved
  hipStream_t st = pgpu_ctx_stream(ctx);
  const uint32_t np = (uint32_t)p->n_pat;
  const PairIndexView& ix = p->ix;
  const ProfRange range("candidates");
  if (!p->d_cand_res) {
    PLAN_NEED(p->d_cand_res = plan_alloc<pgpu_cand_result>(p, SLOT_CAND_RES, np));
    PLAN_NEED(p->d_cand_cnt = plan_alloc<uint32_t>(p, SLOT_CAND_CNT, (size_t)np + 1));
    PLAN_NEED(p->d_cand_first = plan_alloc<unsigned long long>(p, SLOT_CAND_FIRST, (size_t)np + 1));
    PLAN_TRY(plan_events(p, EV_CAND, 2));
  }
  PLAN_TRY(drive_record(p->ev, EV_CAND, st));
  pgpu_cand_launch_count(p->d_meg_out, p->d_meg_off, np, ix.T, ix.n, prm, p->d_cand_res, p->d_cand_cnt, st);
  unsigned long long total = 0;
  PLAN_TRY(scan_total(ctx, p, p->d_cand_cnt, p->d_cand_first, np, nullptr, &total));
  PLAN_NEED(p->d_cand_exons = plan_grow(p, p->d_cand_exons, &p->cand_exons_cap, (size_t)total, (size_t)total / 8 + 256, SLOT_CAND_EXONS));
  pgpu_cand_launch_write(p->d_meg_out, p->d_meg_off, np, ix.T, ix.n, prm, p->d_cand_res, p->d_cand_first, p->d_cand_exons, st);
  PLAN_TRY(drive_record(p->ev, EV_CAND + 1, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  PLAN_TRY(hipGetLastError());
  elapsed_pairs(p, EV_CAND, 1, &p->cand_ms);
  p->cand_total = total;
  return reached(p, CANDIDATES);
}

extern "C" uint64_t pgpu_pairing_plan_candidate_exons(const pgpu_pairing_plan* p) { return p ? p->cand_total : 0; }
extern "C" double pgpu_pairing_plan_candidates_ms(const pgpu_pairing_plan* p) { return p ? p->cand_ms : 0.0; }

extern "C" int pgpu_pairing_plan_fetch_candidates(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_cand_result* out, pgpu_factor* exons,
                                                  size_t exons_cap) {
  if (!ctx || !p || (p->n_pat && !out) || (exons_cap && !exons)) return PGPU_EINVAL;
  if (p->stage < CANDIDATES) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_candidates needs pgpu_pairing_plan_run_candidates first");
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (exons_cap < p->cand_total) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0) return PGPU_OK;
  PLAN_TRY(hipMemcpyAsync(out, p->d_cand_res, p->n_pat * sizeof(pgpu_cand_result), hipMemcpyDeviceToHost, st));
  if (p->cand_total) PLAN_TRY(hipMemcpyAsync(exons, p->d_cand_exons, (size_t)p->cand_total * sizeof(pgpu_factor), hipMemcpyDeviceToHost, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- every candidate of every record that pgpu_pairing_plan_run_meg left in HBM (pgpu_enum.hip); beside the ladder ----
extern "C" int pgpu_pairing_plan_run_candidate_lists(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_cand_params* prm) {
  if (!ctx || !p || !prm) return PGPU_EINVAL;
  p->lists_cands = p->lists_exons = 0; p->lists_ms = 0.f;
  p->lists_valid = p->flists_valid = false;            // its own results are gone, even when the call is then refused
  if (prm->min_factor_len == 0 || prm->min_factor_len > (1u << 24))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad candidate parameters (min_factor_len 0 or above 2^24)");
  if (p->n_pat == 0) { p->lists_valid = true; return PGPU_OK; }
  if (p->stage < RECORDS || p->meg_L != prm->min_factor_len)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_candidate_lists needs the records of pgpu_pairing_plan_run_meg with the same min_factor_len");
  if (const int rc = still_owns(ctx, p, "records")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  const uint32_t np = (uint32_t)p->n_pat;
  const PairIndexView& ix = p->ix;
  const ProfRange range("candidate lists");
  const EnumLayout E = enum_layout(0, np, 0);
  PLAN_NEED(p->d_lists = stage_block(p, p->d_lists, &p->lists_cap, E.total, SLOT_ENUM));
  PLAN_TRY(plan_events(p, EV_LISTS, 2));
  pgpu_enum_result* const d_res = (pgpu_enum_result*)(p->d_lists + E.res);
  uint32_t* const d_cnt_c = (uint32_t*)(p->d_lists + E.cnt_c);
  uint32_t* const d_cnt_e = (uint32_t*)(p->d_lists + E.cnt_e);
  unsigned long long* const d_off_c = (unsigned long long*)(p->d_lists + E.off_c);
  unsigned long long* const d_off_e = (unsigned long long*)(p->d_lists + E.off_e);
  PLAN_TRY(drive_record(p->ev, EV_LISTS, st));
  PLAN_TRY(pgpu_enum_launch_count(p->d_meg_out, p->d_meg_off, np, ix.T, ix.n, prm, d_res, d_cnt_c, d_cnt_e, st));
  unsigned long long total_c = 0, total_e = 0;
  PLAN_TRY(drive_scan(d_cnt_c, d_off_c, np, p->d_tmp, st));
  PLAN_TRY(hipMemcpyAsync(&total_c, d_off_c + np, sizeof total_c, hipMemcpyDeviceToHost, st));
  PLAN_TRY(scan_total(ctx, p, d_cnt_e, d_off_e, np, nullptr, &total_e));
  if (!enum_totals_fit(total_c, total_e))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^32 - 1 candidates or exons in one plan");
  const EnumOutLayout O = enum_out_layout((size_t)total_c, (size_t)total_e);
  PLAN_NEED(p->d_lists_out = stage_block(p, p->d_lists_out, &p->lists_out_cap, O.total, SLOT_ENUM_OUT));
  PLAN_TRY(pgpu_enum_launch_write(p->d_meg_out, p->d_meg_off, np, ix.T, ix.n, prm, d_res, d_off_c, d_off_e,
                                  (pgpu_enum_candidate*)(p->d_lists_out + O.cands), (pgpu_factor*)(p->d_lists_out + O.exons), st));
  PLAN_TRY(drive_record(p->ev, EV_LISTS + 1, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  PLAN_TRY(hipGetLastError());
  elapsed_pairs(p, EV_LISTS, 1, &p->lists_ms);
  p->lists_cands = total_c; p->lists_exons = total_e;
  p->lists_valid = true;
  return PGPU_OK;
}

extern "C" int pgpu_pairing_plan_candidate_list_counts(const pgpu_pairing_plan* p, uint64_t* n_cands, uint64_t* n_exons) {
  if (!p) return PGPU_EINVAL;
  if (n_cands) *n_cands = p->lists_cands;
  if (n_exons) *n_exons = p->lists_exons;
  return PGPU_OK;
}
extern "C" double pgpu_pairing_plan_candidate_lists_ms(const pgpu_pairing_plan* p) { return p ? p->lists_ms : 0.0; }

extern "C" int pgpu_pairing_plan_fetch_candidate_lists(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_enum_result* out,
                                                       pgpu_enum_candidate* cands, size_t cands_cap, pgpu_factor* exons,
                                                       size_t exons_cap) {
  if (!ctx || !p || (p->n_pat && !out) || (cands_cap && !cands) || (exons_cap && !exons)) return PGPU_EINVAL;
  if (const int rc = still_owns(ctx, p, "candidate lists")) return rc;
  if (!p->lists_valid)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_candidate_lists needs pgpu_pairing_plan_run_candidate_lists behind the last run and run_meg");
  if (cands_cap < p->lists_cands) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "candidate buffer too small");
  if (exons_cap < p->lists_exons) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0) return PGPU_OK;
  const EnumLayout E = enum_layout(0, p->n_pat, 0);
  const EnumOutLayout O = enum_out_layout((size_t)p->lists_cands, (size_t)p->lists_exons);
  PLAN_TRY(hipMemcpyAsync(out, p->d_lists + E.res, p->n_pat * sizeof(pgpu_enum_result), hipMemcpyDeviceToHost, st));
  if (p->lists_cands)
    PLAN_TRY(hipMemcpyAsync(cands, p->d_lists_out + O.cands, (size_t)p->lists_cands * sizeof(pgpu_enum_candidate), hipMemcpyDeviceToHost, st));
  if (p->lists_exons)
    PLAN_TRY(hipMemcpyAsync(exons, p->d_lists_out + O.exons, (size_t)p->lists_exons * sizeof(pgpu_factor), hipMemcpyDeviceToHost, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- the candidate lists of the last run_candidate_lists to lists of factorizations, where they lie (pgpu_flists.hip);
// beside the ladder ----
extern "C" int pgpu_pairing_plan_run_factorization_lists(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_flist_params* prm) {
  if (!ctx || !p || !prm) return PGPU_EINVAL;
  p->flist_facts = p->flist_exons = 0;
  for (auto& m : p->flist_ms) m = 0.f;
  p->flists_valid = false;                             // its own results are gone, even when the call is then refused
  if (!flist_params_ok(*prm))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad factorization-list parameters (a setting outside its range, or reserved != 0)");
  if (p->n_pat == 0) { p->flists_valid = true; return PGPU_OK; }
  if (!p->lists_valid)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_factorization_lists needs the candidate lists of pgpu_pairing_plan_run_candidate_lists");
  if (const int rc = still_owns(ctx, p, "candidate lists")) return rc;
  if (p->n_pat > 0x7fffffffull || p->lists_cands > 0x7fffffffull || p->lists_exons > 0x7fffffffull)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 patterns, candidates or candidate exons in one plan");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  if (p->resident) p->d_flist_ws = nullptr;                                    // taken anew, as the block: the pool may have moved
  const ProfRange range("factorization lists");
  const FlistLayout L = flist_layout(p->n_pat, (size_t)p->lists_cands, (size_t)p->lists_exons, pgpu_scan_tmp_bytes(p->n_pat + 1));
  PLAN_NEED(p->d_flist = stage_block(p, p->d_flist, &p->flist_cap, L.total, SLOT_FLIST));
  PLAN_TRY(plan_events(p, EV_FLISTS, 10));
  const EnumLayout E = enum_layout(0, p->n_pat, 0);
  const EnumOutLayout O = enum_out_layout((size_t)p->lists_cands, (size_t)p->lists_exons);
  pgpu_flist_job job;
  job.T = p->ix.T; job.tlen = p->ix.n; job.ests = p->d_pats;
  job.q = nullptr; job.pat_off = p->d_pat_off; job.enum_res = (const pgpu_enum_result*)(p->d_lists + E.res);
  job.cands = (const pgpu_enum_candidate*)(p->d_lists_out + O.cands); job.cand_exons = (const pgpu_factor*)(p->d_lists_out + O.exons);
  job.n = (uint32_t)p->n_pat; job.n_cands = (uint32_t)p->lists_cands; job.n_exons_total = (uint32_t)p->lists_exons;
  job.block = p->d_flist;
  job.ws_alloc = [](void* user, size_t bytes) -> void* {
    pgpu_pairing_plan* q = (pgpu_pairing_plan*)user;
    return q->d_flist_ws = plan_grow(q, q->d_flist_ws, &q->flist_ws_cap, bytes, 0, SLOT_FLIST_WS);
  };
  job.ws_user = p;
  for (int k = 0; k < 10; ++k) job.ev[k] = p->ev[EV_FLISTS + k];
  job.given_gaps = nullptr;
  PLAN_TRY(pgpu_flist_drive(ctx, job, *prm));
  if (job.undersized) return pgpu_clean_undersized(ctx, "factorization lists");
  p->flist_cands = p->lists_cands; p->flist_cand_exons = p->lists_exons;
  p->flist_facts = job.total_facts; p->flist_exons = job.total_exons;
  elapsed_pairs(p, EV_FLISTS, 5, p->flist_ms);
  p->flists_valid = true;
  return PGPU_OK;
}

extern "C" int pgpu_pairing_plan_factorization_list_counts(const pgpu_pairing_plan* p, uint64_t* n_facts, uint64_t* n_exons) {
  if (!p) return PGPU_EINVAL;
  if (n_facts) *n_facts = p->flist_facts;
  if (n_exons) *n_exons = p->flist_exons;
  return PGPU_OK;
}
extern "C" double pgpu_pairing_plan_factorization_lists_ms(const pgpu_pairing_plan* p, int k) {
  return (p && k >= 0 && k < 5) ? p->flist_ms[k] : 0.0;
}

extern "C" int pgpu_pairing_plan_fetch_factorization_lists(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_flist_result* out,
                                                           pgpu_flist_fact* facts, size_t facts_cap, pgpu_factor* exons,
                                                           uint8_t* steps, size_t exons_cap) {
  if (!ctx || !p || (p->n_pat && !out) || (facts_cap && !facts) || (exons_cap && (!exons || !steps))) return PGPU_EINVAL;
  if (const int rc = still_owns(ctx, p, "factorization lists")) return rc;
  if (!p->flists_valid)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_factorization_lists needs pgpu_pairing_plan_run_factorization_lists behind the last "
                                           "run, run_meg and run_candidate_lists");
  if (facts_cap < p->flist_facts) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "factorization buffer too small");
  if (exons_cap < p->flist_exons) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0) return PGPU_OK;
  const FlistLayout L = flist_layout(p->n_pat, (size_t)p->flist_cands, (size_t)p->flist_cand_exons, pgpu_scan_tmp_bytes(p->n_pat + 1));
  PLAN_TRY(hipMemcpyAsync(out, p->d_flist + L.res, p->n_pat * sizeof *out, hipMemcpyDeviceToHost, st));
  if (p->flist_facts)
    PLAN_TRY(hipMemcpyAsync(facts, p->d_flist + L.facts, (size_t)p->flist_facts * sizeof *facts, hipMemcpyDeviceToHost, st));
  if (p->flist_exons) {
    PLAN_TRY(hipMemcpyAsync(exons, p->d_flist + L.out_exons, (size_t)p->flist_exons * sizeof(pgpu_factor), hipMemcpyDeviceToHost, st));
    PLAN_TRY(hipMemcpyAsync(steps, p->d_flist + L.out_steps, (size_t)p->flist_exons, hipMemcpyDeviceToHost, st));
  }
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- every candidate of the last run_candidates through clean, gaps and refine, where it lies (pgpu_fact.hip) -----
extern "C" int pgpu_pairing_plan_run_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_fact_params* prm) {
  if (!ctx || !p || !prm) return PGPU_EINVAL;
  p->fact_total = 0;
  for (auto& m : p->fact_ms) m = 0.f;
  lower(p, CANDIDATES);
  if (!fact_params_ok(*prm)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, FACT_BAD_PARAMS);
  if (p->stage < CANDIDATES)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_factorizations needs the candidates of pgpu_pairing_plan_run_candidates");
  if (p->n_pat == 0) return reached(p, FACTORIZATIONS);
  if (const int rc = still_owns(ctx, p, "candidates")) return rc;
  if (p->n_pat > 0x7fffffffull || p->cand_total > 0x7fffffffull)          // as the index form: exon indices are 32 bits wide
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 patterns or candidate exons in one plan");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  if (p->resident) p->d_fact_ws = nullptr;                                     // taken anew, as the block: the pool may have moved
  const ProfRange range("factorizations");
  const FactLayout L = fact_layout(p->n_pat, (size_t)p->cand_total, pgpu_scan_tmp_bytes(p->n_pat + 1));
  PLAN_NEED(p->d_fact = stage_block(p, p->d_fact, &p->fact_cap, L.total, SLOT_FACT));
  PLAN_TRY(plan_events(p, EV_FACT, 8));
  pgpu_fact_job job;
  job.T = p->ix.T; job.tlen = p->ix.n; job.ests = p->d_pats;
  job.fq = nullptr; job.pat_off = p->d_pat_off; job.cand = p->d_cand_res; job.cand_exons = p->d_cand_exons;
  job.n = (uint32_t)p->n_pat; job.n_exons_total = (uint32_t)p->cand_total;
  job.block = p->d_fact;
  job.ws_alloc = [](void* user, size_t bytes) -> void* {
    pgpu_pairing_plan* q = (pgpu_pairing_plan*)user;
    return q->d_fact_ws = plan_grow(q, q->d_fact_ws, &q->fact_ws_cap, bytes, 0, SLOT_FACT_WS);
  };
  job.ws_user = p;
  for (int k = 0; k < 8; ++k) job.ev[k] = p->ev[EV_FACT + k];
  PLAN_TRY(pgpu_fact_drive(ctx, job, *prm));
  if (job.undersized) return pgpu_clean_undersized(ctx, "factorizations");
  p->fact_total = job.total;
  elapsed_pairs(p, EV_FACT, 4, p->fact_ms);
  return reached(p, FACTORIZATIONS);
}

extern "C" uint64_t pgpu_pairing_plan_factorization_exons(const pgpu_pairing_plan* p) { return p ? p->fact_total : 0; }
extern "C" double pgpu_pairing_plan_factorizations_ms(const pgpu_pairing_plan* p, int k) {
  return (p && k >= 0 && k < 4) ? p->fact_ms[k] : 0.0;
}

extern "C" int pgpu_pairing_plan_fetch_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_fact_result* out, pgpu_factor* exons,
                                                      uint8_t* steps, size_t cap) {
  if (!ctx || !p || (p->n_pat && !out) || (cap && (!exons || !steps))) return PGPU_EINVAL;
  if (p->stage < FACTORIZATIONS) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_factorizations needs pgpu_pairing_plan_run_factorizations first");
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (cap < p->fact_total) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0) return PGPU_OK;
  const FactLayout L = fact_layout(p->n_pat, (size_t)p->cand_total, pgpu_scan_tmp_bytes(p->n_pat + 1));
  PLAN_TRY(drive_download(p->d_fact, L, p->n_pat * sizeof *out, p->fact_total, out, exons, steps, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- the factorizations of the last run_factorizations through tail and small, where they lie (pgpu_final.hip) --------
static int run_final_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_small_params* prm, const bool wide) {
  if (!ctx || !p || !prm) return PGPU_EINVAL;
  p->final_total = 0;
  for (auto& m : p->final_ms) m = 0.f;
  lower(p, FACTORIZATIONS);
  if (!small_params_ok(prm)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, SMALL_BAD_PARAMS);
  if (p->stage < FACTORIZATIONS)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_final_factorizations needs the factorizations of pgpu_pairing_plan_run_factorizations");
  if (p->n_pat == 0) return reached(p, FINALS);
  if (const int rc = still_owns(ctx, p, "factorizations")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  ClassView cv;
  if (const int rc = pgpu_class_view_get(ctx, p->idx, &cv)) return rc;
  const ProfRange range("final factorizations");
  const FinalLayout L = final_layout(p->n_pat, (size_t)p->cand_total, pgpu_scan_tmp_bytes(p->n_pat + 1));
  PLAN_NEED(p->d_final = stage_block(p, p->d_final, &p->final_cap, L.total, SLOT_FINAL));
  PLAN_TRY(plan_events(p, EV_FINAL, 6));
  pgpu_final_job job;
  job.ix = pgpu_index_small_view(p->idx); job.cv = &cv;
  job.ests = p->d_pats; job.ests_len = p->seq_bytes;
  job.fq = nullptr; job.pat_off = p->d_pat_off; job.orig_off = p->d_orig_off;
  job.n = (uint32_t)p->n_pat; job.n_exons_total = (uint32_t)p->cand_total; job.min_intron_length = prm->min_intron_length;
  job.fact_block = p->d_fact; job.block = p->d_final; job.wide = wide;
  for (int k = 0; k < 6; ++k) job.ev[k] = p->ev[EV_FINAL + k];
  PLAN_TRY(pgpu_final_drive(ctx, job));
  p->final_total = job.total;
  elapsed_pairs(p, EV_FINAL, 3, p->final_ms);
  return reached(p, FINALS);
}

extern "C" int pgpu_pairing_plan_run_final_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_small_params* prm) {
  return run_final_factorizations(ctx, p, prm, false);
}
// the same rung with the wide kernels behind the two stage kernels (pgpu_final_job::wide)
extern "C" int pgpu_pairing_plan_run_final_factorizations_wide(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_small_params* prm) {
  return run_final_factorizations(ctx, p, prm, true);
}

extern "C" uint64_t pgpu_pairing_plan_final_exons(const pgpu_pairing_plan* p) { return p ? p->final_total : 0; }
extern "C" double pgpu_pairing_plan_final_ms(const pgpu_pairing_plan* p, int k) { return (p && k >= 0 && k < 3) ? p->final_ms[k] : 0.0; }

extern "C" int pgpu_pairing_plan_fetch_final_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_final_result* out,
                                                            pgpu_factor* exons, uint8_t* steps, size_t cap) {
  if (!ctx || !p || (p->n_pat && !out) || (cap && (!exons || !steps))) return PGPU_EINVAL;
  if (p->stage < FINALS)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_final_factorizations needs pgpu_pairing_plan_run_final_factorizations first");
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (cap < p->final_total) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0) return PGPU_OK;
  const FinalLayout L = final_layout(p->n_pat, (size_t)p->cand_total, pgpu_scan_tmp_bytes(p->n_pat + 1));
  PLAN_TRY(drive_download(p->d_final, L, p->n_pat * sizeof *out, p->final_total, out, exons, steps, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- the finals of the last run_final_factorizations to one verdict per unit and est-fact's groups (pgpu_unit.hip) -----
extern "C" int pgpu_pairing_plan_run_units(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_unit_query* q, size_t n_units,
                                           const pgpu_unit_params* prm) {
  if (!ctx || !p || !prm || (n_units && !q)) return PGPU_EINVAL;
  p->unit_total = 0; p->n_units = 0; p->unit_ms = 0.f;
  lower(p, FINALS);
  if (const char* wrong = unit_params_wrong(*prm)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (n_units > UNIT_MAX_COUNT || p->n_pat > UNIT_MAX_COUNT) return pgpu_ctx_fail(ctx, PGPU_EINVAL, UNIT_TOO_MANY);
  {
    const std::unique_ptr<uint8_t, void (*)(void*)> named((uint8_t*)calloc(p->n_pat ? p->n_pat : 1, 1), free);
    if (!named) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "no memory for the table of the patterns the units name");
    if (const char* wrong = unit_queries_wrong(q, n_units, p->n_pat, named.get())) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  }
  if (p->stage < FINALS)
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_units needs the finals of pgpu_pairing_plan_run_final_factorizations");
  if (p->n_pat == 0 || n_units == 0) return reached(p, UNITS);
  if (const int rc = still_owns(ctx, p, "finals")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  const ProfRange range("units");
  const UnitLayout L = unit_layout(n_units, (size_t)p->final_total, pgpu_scan_tmp_bytes(n_units + 1));
  PLAN_NEED(p->d_unit = stage_block(p, p->d_unit, &p->unit_cap, L.total, SLOT_UNITS));
  PLAN_TRY(plan_events(p, EV_UNITS, 2));
  const FinalLayout F = final_layout(p->n_pat, (size_t)p->cand_total, pgpu_scan_tmp_bytes(p->n_pat + 1));
  PLAN_TRY(hipMemcpyAsync(p->d_unit + L.q, q, n_units * sizeof *q, hipMemcpyHostToDevice, pgpu_ctx_stream(ctx)));
  pgpu_unit_job job;
  job.res = (const pgpu_final_result*)(p->d_final + F.res); job.exons = (const pgpu_factor*)(p->d_final + F.out_exons);
  job.n_exons_total = (uint32_t)p->final_total; job.n_done_exons = (size_t)p->final_total;
  job.empty = nullptr; job.recs = p->d_meg_out; job.rec_first = p->d_meg_off;
  job.params = *prm; job.n = (uint32_t)n_units; job.block = p->d_unit;
  job.ev[0] = p->ev[EV_UNITS]; job.ev[1] = p->ev[EV_UNITS + 1];
  PLAN_TRY(pgpu_unit_drive(ctx, job));
  p->unit_total = job.total; p->n_units = n_units;
  elapsed_pairs(p, EV_UNITS, 1, &p->unit_ms);
  return reached(p, UNITS);
}

extern "C" uint64_t pgpu_pairing_plan_unit_bytes(const pgpu_pairing_plan* p) { return p ? p->unit_total : 0; }
extern "C" double pgpu_pairing_plan_units_ms(const pgpu_pairing_plan* p) { return p ? p->unit_ms : 0.0; }

extern "C" int pgpu_pairing_plan_fetch_units(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_unit_result* out, void* blob, size_t cap) {
  if (!ctx || !p || (p->n_units && !out) || (cap && !blob)) return PGPU_EINVAL;
  if (p->stage < UNITS) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_units needs pgpu_pairing_plan_run_units first");
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (cap < p->unit_total) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "blob too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_units == 0) return PGPU_OK;
  const UnitLayout L = unit_layout(p->n_units, (size_t)p->final_total, pgpu_scan_tmp_bytes(p->n_units + 1));
  PLAN_TRY(hipMemcpyAsync(out, p->d_unit + L.out, p->n_units * sizeof(pgpu_unit_result), hipMemcpyDeviceToHost, st));
  if (p->unit_total) PLAN_TRY(hipMemcpyAsync(blob, p->d_unit + L.blob, (size_t)p->unit_total, hipMemcpyDeviceToHost, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}

// ---- the units of the last run_units to est-fact's two text files, where they lie (pgpu_text.hip) -----------------------
extern "C" int pgpu_pairing_plan_run_texts(pgpu_ctx* ctx, pgpu_pairing_plan* p, const pgpu_text_source* src, const char* headers,
                                           size_t headers_len, const uint64_t* hdr_first) {
  if (!ctx || !p || !src || (p->n_units && !hdr_first) || (headers_len && !headers)) return PGPU_EINVAL;
  p->text_raw_total = p->text_pests_total = 0; p->text_ms = p->text_write_ms = 0.f; p->text_timed = false;
  lower(p, UNITS);
  if (src->owner != ctx) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "this text source was made on another context");
  if (p->stage < UNITS) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_texts needs the units of pgpu_pairing_plan_run_units");
  const size_t n_units = p->n_units;
  if (hdr_first)
    if (const char* wrong = text_offsets_wrong(hdr_first, n_units, headers_len, TEXT_BAD_HDR)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (p->n_pat == 0 || n_units == 0) return reached(p, TEXTS);
  if (const int rc = still_owns(ctx, p, "units")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  const ProfRange range("texts");
  hipStream_t st = pgpu_ctx_stream(ctx);
  const TextLayout L = text_layout(n_units, headers_len, pgpu_scan_tmp_bytes(n_units + 1));
  PLAN_NEED(p->d_text = stage_block(p, p->d_text, &p->text_cap, L.total, SLOT_TEXTS));
  PLAN_TRY(plan_events(p, EV_TEXTS, 3));
  // the headers are uploaded at every run: about 30 bytes per unit
  if (headers_len) PLAN_TRY(hipMemcpyAsync(p->d_text + L.hdr, headers, headers_len, hipMemcpyHostToDevice, st));
  PLAN_TRY(hipMemcpyAsync(p->d_text + L.hdr_first, hdr_first, (n_units + 1) * sizeof *hdr_first, hipMemcpyHostToDevice, st));
  const UnitLayout U = unit_layout(n_units, (size_t)p->final_total, pgpu_scan_tmp_bytes(n_units + 1));
  pgpu_text_job job;
  job.units = (const pgpu_unit_result*)(p->d_unit + U.out); job.n = (uint32_t)n_units;
  job.blob = p->d_unit + U.blob; job.blob_len = p->unit_total; job.headers_len = headers_len;
  job.seqs = p->d_pats; job.seq_at = p->d_orig_off; job.seq_off = p->d_pat_off; job.n_pat = (uint32_t)p->n_pat;
  job.genomic = src->d; job.genomic_len = src->len;
  job.block = p->d_text;
  for (int k = 0; k < 3; ++k) job.ev[k] = p->ev[EV_TEXTS + k];
  PLAN_TRY(pgpu_text_count(ctx, job));                 // the call's one host wait
  const size_t raw = (size_t)job.raw_total, pests = (size_t)job.pests_total, o_pests = up256(raw ? raw : 1);
  PLAN_NEED(p->d_text_blobs = stage_block(p, p->d_text_blobs, &p->text_blobs_cap, o_pests + up256(pests ? pests : 1), SLOT_TEXT_BLOBS));
  PLAN_TRY(pgpu_text_write(ctx, job, p->d_text_blobs, p->d_text_blobs + o_pests));
  p->text_raw_total = job.raw_total; p->text_pests_total = job.pests_total; p->text_pests_at = o_pests;
  p->text_headers_len = headers_len; p->text_timed = p->ev[EV_TEXTS] != nullptr;
  return reached(p, TEXTS);
}

extern "C" uint64_t pgpu_pairing_plan_text_bytes(const pgpu_pairing_plan* p, int which) {
  return !p ? 0 : which == 0 ? p->text_raw_total : which == 1 ? p->text_pests_total : 0;
}
// the run did not wait for its write pass: the first question about its time does
static void text_times(pgpu_pairing_plan* p) {
  if (!p->text_timed || p->stage < TEXTS) return;
  p->text_timed = false;
  if (hipEventSynchronize(p->ev[EV_TEXTS + 1]) != hipSuccess) return;
  elapsed_pairs(p, EV_TEXTS, 1, &p->text_ms);
  hipEventElapsedTime(&p->text_write_ms, p->ev[EV_TEXTS + 2], p->ev[EV_TEXTS + 1]);
}
extern "C" double pgpu_pairing_plan_texts_ms(pgpu_pairing_plan* p) {
  if (!p) return 0.0;
  text_times(p);
  return p->text_ms;
}
extern "C" double pgpu_pairing_plan_texts_write_ms(pgpu_pairing_plan* p) {
  if (!p) return 0.0;
  text_times(p);
  return p->text_write_ms;
}

extern "C" int pgpu_pairing_plan_fetch_texts(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_text_result* out, void* raw, size_t raw_cap,
                                             void* pests, size_t pests_cap) {
  if (!ctx || !p || (raw_cap && !raw) || (pests_cap && !pests)) return PGPU_EINVAL;
  if (p->stage < TEXTS) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_texts needs pgpu_pairing_plan_run_texts first");
  if (p->n_pat && p->n_units && !out) return PGPU_EINVAL;
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (raw_cap < p->text_raw_total || pests_cap < p->text_pests_total) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "text buffers too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0 || p->n_units == 0) return PGPU_OK;
  const TextLayout L = text_layout(p->n_units, p->text_headers_len, pgpu_scan_tmp_bytes(p->n_units + 1));
  PLAN_TRY(hipMemcpyAsync(out, p->d_text + L.out, p->n_units * sizeof(pgpu_text_result), hipMemcpyDeviceToHost, st));
  if (p->text_raw_total) PLAN_TRY(hipMemcpyAsync(raw, p->d_text_blobs, (size_t)p->text_raw_total, hipMemcpyDeviceToHost, st));
  if (p->text_pests_total)
    PLAN_TRY(hipMemcpyAsync(pests, p->d_text_blobs + p->text_pests_at, (size_t)p->text_pests_total, hipMemcpyDeviceToHost, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  PLAN_TRY(hipGetLastError());
  return PGPU_OK;
}

// ---- the records of the units of the last run_units to est-fact's three side files, where they lie (pgpu_side.hip) -------
extern "C" int pgpu_pairing_plan_run_sides(pgpu_ctx* ctx, pgpu_pairing_plan* p) {
  if (!ctx || !p) return PGPU_EINVAL;
  p->side_total[0] = p->side_total[1] = p->side_total[2] = 0; p->side_ms = p->side_write_ms = 0.f; p->side_timed = false;
  lower(p, TEXTS);
  if (p->stage < TEXTS) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "run_sides needs the headers of pgpu_pairing_plan_run_texts");
  const size_t n_units = p->n_units;
  if (p->n_pat == 0 || n_units == 0) return reached(p, SIDES);
  if (const int rc = still_owns(ctx, p, "texts")) return rc;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  const ProfRange range("sides");
  const SideLayout L = side_layout(n_units, pgpu_scan_tmp_bytes(n_units + 1));
  PLAN_NEED(p->d_side = stage_block(p, p->d_side, &p->side_cap, L.total, SLOT_SIDES));
  PLAN_TRY(plan_events(p, EV_SIDES, 3));
  const UnitLayout U = unit_layout(n_units, (size_t)p->final_total, pgpu_scan_tmp_bytes(n_units + 1));
  const TextLayout T = text_layout(n_units, p->text_headers_len, pgpu_scan_tmp_bytes(n_units + 1));
  pgpu_side_job job;
  job.q = (const pgpu_unit_query*)(p->d_unit + U.q); job.units = (const pgpu_unit_result*)(p->d_unit + U.out); job.n = (uint32_t)n_units;
  job.recs = p->d_meg_out; job.recs_len = p->meg_total; job.rec_first = p->d_meg_off; job.n_pat = (uint32_t)p->n_pat;
  job.hdr = p->d_text + T.hdr; job.hdr_first = (const unsigned long long*)(p->d_text + T.hdr_first);
  job.seqs = p->d_pats; job.seq_at = p->d_orig_off; job.seq_off = p->d_pat_off;
  job.block = p->d_side;
  for (int k = 0; k < 3; ++k) job.ev[k] = p->ev[EV_SIDES + k];
  PLAN_TRY(pgpu_side_count(ctx, job));                 // the call's one host wait
  const SideBlobs S = side_blobs(job.total);
  PLAN_NEED(p->d_side_blobs = stage_block(p, p->d_side_blobs, &p->side_blobs_cap, S.total, SLOT_SIDE_BLOBS));
  PLAN_TRY(pgpu_side_write(ctx, job, p->d_side_blobs + S.at[0], p->d_side_blobs + S.at[1], p->d_side_blobs + S.at[2]));
  for (int k = 0; k < 3; ++k) p->side_total[k] = job.total[k];
  p->side_timed = p->ev[EV_SIDES] != nullptr;
  return reached(p, SIDES);
}

extern "C" uint64_t pgpu_pairing_plan_side_bytes(const pgpu_pairing_plan* p, int which) {
  return (p && which >= 0 && which < 3) ? p->side_total[which] : 0;
}
// the run did not wait for its write pass: the first question about its time does
static void side_times(pgpu_pairing_plan* p) {
  if (!p->side_timed || p->stage < SIDES) return;
  p->side_timed = false;
  if (hipEventSynchronize(p->ev[EV_SIDES + 1]) != hipSuccess) return;
  elapsed_pairs(p, EV_SIDES, 1, &p->side_ms);
  hipEventElapsedTime(&p->side_write_ms, p->ev[EV_SIDES + 2], p->ev[EV_SIDES + 1]);
}
extern "C" double pgpu_pairing_plan_sides_ms(pgpu_pairing_plan* p) {
  if (!p) return 0.0;
  side_times(p);
  return p->side_ms;
}
extern "C" double pgpu_pairing_plan_sides_write_ms(pgpu_pairing_plan* p) {
  if (!p) return 0.0;
  side_times(p);
  return p->side_write_ms;
}

extern "C" int pgpu_pairing_plan_fetch_sides(pgpu_ctx* ctx, pgpu_pairing_plan* p, pgpu_side_result* out, void* megs, size_t megs_cap,
                                             void* pmegs, size_t pmegs_cap, void* edges, size_t edges_cap) {
  if (!ctx || !p || (megs_cap && !megs) || (pmegs_cap && !pmegs) || (edges_cap && !edges)) return PGPU_EINVAL;
  if (p->stage < SIDES) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "fetch_sides needs pgpu_pairing_plan_run_sides first");
  if (p->n_pat && p->n_units && !out) return PGPU_EINVAL;
  if (const int rc = still_owns(ctx, p, "results")) return rc;
  if (megs_cap < p->side_total[0] || pmegs_cap < p->side_total[1] || edges_cap < p->side_total[2])
    return pgpu_ctx_fail(ctx, PGPU_ENOSPC, SIDE_NO_SPACE);
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (p->n_pat == 0 || p->n_units == 0) return PGPU_OK;
  const SideLayout L = side_layout(p->n_units, pgpu_scan_tmp_bytes(p->n_units + 1));
  const SideBlobs S = side_blobs(p->side_total);
  PLAN_TRY(hipMemcpyAsync(out, p->d_side + L.out, p->n_units * sizeof(pgpu_side_result), hipMemcpyDeviceToHost, st));
  void* const dst[3] = { megs, pmegs, edges };
  for (int k = 0; k < 3; ++k)
    if (p->side_total[k]) PLAN_TRY(hipMemcpyAsync(dst[k], p->d_side_blobs + S.at[k], (size_t)p->side_total[k], hipMemcpyDeviceToHost, st));
  PLAN_TRY(pgpu_ctx_wait(ctx));
  PLAN_TRY(hipGetLastError());
  return PGPU_OK;
}

// ---- one-shot: create, run, fetch, destroy -----------------------------------------------------------------------
extern "C" int pgpu_pairings(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns,
                             const uint64_t* pat_off, size_t n_pat, const pgpu_pairing_params* params,
                             pgpu_pairing* out, size_t out_cap, uint64_t* out_first, size_t* n_out) {
  pgpu_pairing_plan* p = nullptr;
  int rc = pgpu_pairing_plan_create(ctx, idx, patterns, pat_off, n_pat, &p);
  if (rc != PGPU_OK) return rc;
  rc = pgpu_pairing_plan_run(ctx, p, params);
  if (rc == PGPU_OK) {
    if (n_out) *n_out = (size_t)p->n_out;
    rc = pgpu_pairing_plan_fetch(ctx, p, out, out_cap, out_first);
  }
  pgpu_pairing_plan_destroy(ctx, p);
  return rc;
}
