// The intron-border decision of refine_intron (src/refine-intron.c:47-265) as one wave runs it on rows staged in LDS:
// what refine_kernel (pgpu_refine.hip, one query per wave) and chain_kernel (pgpu_chain.hip, one chain of introns per
// wave) share.  The division of the work over the lanes is described at the top of pgpu_refine.hip.
#pragma once

#include "pgpu_index.h"

namespace {

constexpr int MAX_DIM = PGPU_REFINE_MAX_DIM;
constexpr int MAX_ED = PGPU_REFINE_MAX_ED;

// getBursetFrequency (src/refine-intron.c:376-556) as data, the table of ef_refine_intron.c: index = donor[0], donor[1],
// acceptor[0], acceptor[1] at 2 bits each (A=0 C=1 G=2 T=3)
__constant__ uint8_t c_burset[256] = {
    0,   0,   1,   1,   0,   0,   0,   0,   0,   0,   0,   1,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   1,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   1,   5,   0,   0,   0,   0,   2,   0,   1,   0,   0,   0,   0,   2,   0,
    1,   8,   7,   2,   0,   0,   0,   0,   0,   1,   0,   1,   0,   0,   0,   0,
    0,   0,   1,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   1,
    0,   0,   2,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   1,   0,   1,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   2,   0,   0,   1,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   8,   0,   0,   0,   0,   0,   0,   0,   0,   1,   0,   1,   1,   0,
    0,   0, 126,   0,   0,   0,   0,   0,   0,   0,   1,   0,   1,   0,   0,   0,
    0,   1,  11,   0,   1,   0,   0,   0,   2,   0,   0,   0,   0,   2,   0,   0,
    0,   4, 200,   2,   9,   0,   4,   3,   0,   1,  10,   1,   7,   2,   8,   2,
    0,   0,   6,   0,   0,   0,   1,   0,   0,   0,   0,   0,   0,   1,   0,   0,
    0,   0,   1,   0,   0,   0,   0,   0,   0,   0,   1,   0,   0,   0,   0,   0,
    0,   1,   7,   0,   0,   0,   0,   0,   0,   0,   2,   0,   0,   0,   0,   0,
    0,   0,   5,   1,   0,   0,   0,   0,   0,   0,   1,   0,   0,   0,   0,   0,
};

// what one query works on: the staged rows with their strlen, a sequence with its length
struct Rows { const uint8_t* e; const uint8_t* g; int dim, glen, elen, isoa, ieoa; };
struct Seq { const uint8_t* p; int len; };

__device__ __forceinline__ int row_at(const uint8_t* r, int dim, int i) { return (unsigned)i < (unsigned)dim ? (int)r[i] : 0; }
__device__ __forceinline__ int seq_at(const Seq& s, int i) { return (unsigned)i < (unsigned)s.len ? (int)s.p[i] : 0; }

// strlen of a staged row: the first 0 in [0, dim), or dim
__device__ __forceinline__ int row_strlen(const uint8_t* r, int dim, int lane) {
  for (int base = 0; base < dim; base += 64) {
    const int i = base + lane;
    const unsigned long long z = __ballot(i < dim && r[i] == 0);
    if (z) return base + __builtin_ctzll(z);
  }
  return dim;
}

// columns lo .. hi (inclusive) of both rows that hold no '-'; a column outside the rows holds none
__device__ __forceinline__ void count_columns(const Rows& al, int lo, int hi, int lane, int& cg, int& ce) {
  int gaps_g = 0, gaps_e = 0;
  const int a = lo < 0 ? 0 : lo, b = hi < al.dim - 1 ? hi : al.dim - 1;
  for (int base = a; base <= b; base += 64) {
    const int i = base + lane;
    const bool in = i <= b;
    gaps_g += __popcll(__ballot(in && al.g[i] == '-'));
    gaps_e += __popcll(__ballot(in && al.e[i] == '-'));
  }
  const int n = hi >= lo ? hi - lo + 1 : 0;
  cg = n - gaps_g; ce = n - gaps_e;
}

// Find_AG_after_on_the_right (:892-940)
__device__ __forceinline__ void find_AG_after_right(const Rows& al, int init, int lane, int& cut_on_align, int& gen_cut, int& est_cut) {
  cut_on_align = -1; gen_cut = -1; est_cut = -1;
  int index = init - 2;
  if (index < 0 || al.glen == 0) return;          // (size_t)(init - 2) lies beyond every row; an empty row holds nothing
  bool stop = false;
  while (!stop && index < al.glen - 1) {
    while (row_at(al.g, al.dim, index) == '-') ++index;
    const int p0 = row_at(al.g, al.dim, index);
    ++index;
    while (row_at(al.g, al.dim, index) == '-') ++index;
    stop = p0 == 'A' && row_at(al.g, al.dim, index) == 'G';
  }
  if (!stop) return;
  cut_on_align = index + 1;
  count_columns(al, al.ieoa + 1, index, lane, gen_cut, est_cut);
}

// Find_ACCEPTOR_before_on_the_left (:942-990); the pattern is p0 p1
__device__ __forceinline__ void find_before_left(const Rows& al, int init, int p0w, int p1w, int lane, int& cut_on_align, int& gen_cut,
                                                 int& est_cut) {
  cut_on_align = -1; gen_cut = -1; est_cut = -1;
  int index = init + 2;
  bool stop = false;
  while (!stop && index > 0) {
    while (row_at(al.g, al.dim, index) == '-') --index;
    const int p1 = row_at(al.g, al.dim, index);
    --index;
    while (index >= 0 && row_at(al.g, al.dim, index) == '-') --index;
    const int p0 = index < 0 ? 0 : row_at(al.g, al.dim, index);
    stop = p0 == p0w && p1 == p1w;
  }
  if (!stop) return;
  cut_on_align = index - 1;
  count_columns(al, index, al.isoa - 1, lane, gen_cut, est_cut);
}

// Find_ACCEPTOR_after_on_the_left (:1852-1874): the first column c in [init, intron_end_on_align) with the pattern at
// c, c + 1 of the genomic row (gaps are not skipped); the loop leaves index = c + 1
__device__ __forceinline__ int find_after_left(const Rows& al, int init, int p0w, int p1w, int lane) {
  for (int base = init; base < al.ieoa; base += 64) {
    const int c = base + lane;
    const unsigned long long hit = __ballot(c < al.ieoa && row_at(al.g, al.dim, c) == p0w && row_at(al.g, al.dim, c + 1) == p1w);
    if (hit) return base + __builtin_ctzll(hit) + 1 - al.isoa - 1;
  }
  return -1;
}

// Find_AG_before_on_the_right (:1950-1972): the last column c in (intron_start_on_align, init] with AG at c - 1, c; the
// loop leaves index = c - 1
__device__ __forceinline__ int find_AG_before_right(const Rows& al, int init, int lane) {
  for (int top = init; top > al.isoa; top -= 64) {
    const int c = top - lane;
    const unsigned long long hit = __ballot(c > al.isoa && row_at(al.g, al.dim, c - 1) == 'A' && row_at(al.g, al.dim, c) == 'G');
    if (hit) return al.ieoa - (top - __builtin_ctzll(hit) - 1) - 1;
  }
  return -1;
}

// Get_genomic/est_substring_from_alignment (:1878-1948) for the eight-column piece (at most 16 columns): the ungapped
// bytes of the row into `out`, their count returned, the mismatches of the piece in *error.  The caller has checked
// 0 <= init < glen (otherwise the routine returns NULL and leaves *error alone).
__device__ __forceinline__ int row_piece(const Rows& al, bool genomic, int init, int length, int lane, uint8_t* out, int* error) {
  const int rlen = genomic ? al.glen : al.elen;
  const int actual = rlen - init < length ? rlen - init : length;      // <= 16; may be negative: nothing then
  const uint8_t* row = genomic ? al.g : al.e;
  const int i = init + lane;
  const bool in = lane < actual;
  const unsigned long long keep = __ballot(in && row[i] != '-');
  *error = __popcll(__ballot(in && al.g[i] != al.e[i]));
  if (in && row[i] != '-') out[__popcll(keep & ((1ull << lane) - 1ull))] = row[i];
  return __popcll(keep);
}

// real_substring (src/util.c:138-158) as a piece of its sequence: clamped at the start, cut at the end and at a 0
struct Piece { int start, len; };
__device__ __forceinline__ Piece substring(const Seq& s, int index, int length, int lane) {
  if (index < 0) { length += index; index = 0; }
  if (length < 0) length = 0;
  const int room = index < s.len ? s.len - index : 0;
  if (length > room) length = room;
  for (int base = 0; base < length; base += 64) {
    const int k = base + lane;
    const unsigned long long z = __ballot(k < length && s.p[index + k] == 0);
    if (z) { length = base + __builtin_ctzll(z); break; }
  }
  Piece p; p.start = index; p.len = length;
  return p;
}

// one operand of an edit distance into LDS: the piece, with `ext` (next bytes, in LDS) in front of it or behind it.
// Returns its length, or -1 when it exceeds MAX_ED (nothing is written beyond the buffer).
__device__ __forceinline__ int stage_operand(uint8_t* dst, const Seq& s, const Piece& p, const uint8_t* ext, int next, bool ext_first, int lane) {
  const int total = p.len + next;
  if (total > MAX_ED) return -1;
  const int at = ext_first ? next : 0, ext_at = ext_first ? 0 : p.len;
  for (int k = lane; k < p.len; k += 64) dst[at + k] = s.p[p.start + k];
  if (lane < next) dst[ext_at + lane] = ext[lane];
  return total;
}

// Levenshtein distance of A[0..la) and B[0..lb) (both in LDS, at most MAX_ED bytes): diagonal k holds the cells (i, k - i);
// d[0..2] are three diagonals indexed by i.  The block is one wave: the barrier orders its LDS traffic.
__device__ __forceinline__ int wave_edit_distance(const uint8_t* A, int la, const uint8_t* B, int lb, int* d, int lane) {
  if (la == 0) return lb;
  if (lb == 0) return la;
  int *p2 = d, *p1 = d + (MAX_ED + 1), *cur = d + 2 * (MAX_ED + 1);
  for (int k = 0; k <= la + lb; ++k) {
    const int lo = k > lb ? k - lb : 0, hi = k < la ? k : la;
    for (int i = lo + lane; i <= hi; i += 64) {
      const int j = k - i;
      int v;
      if (i == 0) v = j;
      else if (j == 0) v = i;
      else {
        const int up = p1[i - 1] + 1, left = p1[i] + 1, diag = p2[i - 1] + (A[i - 1] != B[j - 1] ? 1 : 0);
        v = up < left ? up : left;
        v = diag < v ? diag : v;
      }
      cur[i] = v;
    }
    __syncthreads();
    int* t = p2; p2 = p1; p1 = cur; cur = t;
  }
  const int r = p1[la];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int base_code(int c) {
  switch (c) {
    case 'A': case 'a': return 0; case 'C': case 'c': return 1;
    case 'G': case 'g': return 2; case 'T': case 't': return 3;
  }
  return -1;
}

// Check_Burset_patterns (:346-360) as ef_check_burset_patterns: two real_substrings of two bytes, then the table
__device__ __forceinline__ int check_burset_patterns(const Seq& gen, int donor_left, int acceptor_right) {
  int c[4];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    int index = w == 0 ? donor_left + 1 : acceptor_right - 2, length = 2;
    if (index < 0) { length += index; index = 0; }
    const int b0 = length > 0 ? seq_at(gen, index) : 0;
    const int b1 = length > 1 && b0 != 0 ? seq_at(gen, index + 1) : 0;
    if (b0 == 0 || b1 == 0) return 0;                 // strlen != 2
    c[2 * w] = base_code(b0); c[2 * w + 1] = base_code(b1);
  }
  if ((c[0] | c[1] | c[2] | c[3]) < 0) return 0;
  return c_burset[(c[0] << 6) | (c[1] << 4) | (c[2] << 2) | c[3]];
}

// Try_Burset_after_match (:267-344); el = strlen of the EST
__device__ __forceinline__ void try_burset_after_match(const Seq& est, const Seq& gen, int el, int& factor_left, int& donor_right,
                                                       int& acc_left, int donor_factor_left, int acc_factor_right) {
  int sf = factor_left, sa = acc_left, sd = donor_right;
  int uf = sf, ua = sa, ud = sd;
  int frequency = 0;
  bool right_to_left = false, stop = false;
  while (!stop && seq_at(est, sf) == seq_at(gen, sa) && sf > donor_factor_left + 1) {
    if (sf == 0 || sd == -1) stop = true;
    else {
      const int f = check_burset_patterns(gen, sd, sa);
      if (f > frequency) { frequency = f; uf = sf; ua = sa; ud = sd; }
      --sf; --sd; --sa;
    }
  }
  sf = factor_left; sa = acc_left + 1; sd = donor_right + 1;
  stop = false;
  while (!stop && seq_at(est, sf) == seq_at(gen, sd) && sf < acc_factor_right) {
    if (sf == el || sa == gen.len) stop = true;
    else {
      const int f = check_burset_patterns(gen, sd, sa);
      if (f > frequency) { frequency = f; uf = sf; ua = sa; ud = sd; right_to_left = true; }
      ++sf; ++sd; ++sa;
    }
  }
  if (right_to_left) uf += 1;
  factor_left = uf; donor_right = ud; acc_left = ua;
}

// LDS of one query (one wave per block)
struct RefineLds {
  uint8_t rows[2 * MAX_DIM];
  uint8_t a[MAX_ED], b[MAX_ED];
  uint8_t ext_est[16], ext_gen[16];
  int diag[3 * (MAX_ED + 1)];
};

// One Shift_* routine (the common body, ef_refine_intron.c:207-342).  r2l: search AG to the right of the intron and the
// donor pattern inside it; variant1: the "_1" rule (GT), else the "_2" rule (GC); the donor pattern is 'G' pat1.
// Returns 1 settled, 0 not settled, -1 an operand exceeds MAX_ED.
__device__ __forceinline__ int shift_generic(RefineLds& L, const Seq& est, const Seq& gen, const Rows& al, int naf, int ndr, int nalg,
                                             bool r2l, bool variant1, int pat1, int lane, int& out_donor_right, int& out_acc_left,
                                             int& out_factor_left) {
  int init_right = r2l ? al.ieoa + 1 : al.ieoa;
  int init_left = r2l ? al.isoa : al.isoa - 1;
  int ext_error = -1, n_ext_est = 0, n_ext_gen = 0;
  bool has_ext;
  {
    int l_substr = 8, start = r2l ? al.isoa - 8 : al.ieoa + 1;
    if (r2l && start < 0) { l_substr = l_substr - start; start = 0; }
    has_ext = start >= 0 && start < al.glen;
    if (has_ext) {
      n_ext_est = row_piece(al, false, start, l_substr, lane, L.ext_est, &ext_error);
      n_ext_gen = row_piece(al, true, start, l_substr, lane, L.ext_gen, &ext_error);
    }
  }
  const bool use_ext = has_ext && ext_error > 0;
  int gen_cut[2], est_cut[2], sub_dim[2];
  Piece cut_factor[2], prev_match[2], match_str[2];
  bool has_cut[2], has_match[2], has_ext_cut[2], has_ext_match[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int cut_on_align;
    if (r2l) find_AG_after_right(al, init_right, lane, cut_on_align, gen_cut[i], est_cut[i]);
    else find_before_left(al, init_left, 'G', pat1, lane, cut_on_align, gen_cut[i], est_cut[i]);
    has_cut[i] = est_cut[i] > -1;
    cut_factor[i].start = cut_factor[i].len = prev_match[i].start = prev_match[i].len = 0;
    if (has_cut[i]) {
      if (r2l) {
        prev_match[i] = substring(gen, nalg, gen_cut[i], lane);
        cut_factor[i] = substring(est, naf, est_cut[i], lane);
        init_right = cut_on_align + 1;
      } else {
        prev_match[i] = substring(gen, ndr - gen_cut[i] + 1, gen_cut[i], lane);
        cut_factor[i] = substring(est, naf - est_cut[i], est_cut[i], lane);
        init_left = cut_on_align - 1;
      }
    }
    has_ext_cut[i] = has_cut[i] && use_ext;
    sub_dim[i] = r2l ? find_after_left(al, init_left, 'G', pat1, lane) : find_AG_before_right(al, init_right, lane);
    has_match[i] = sub_dim[i] > -1;
    match_str[i].start = match_str[i].len = 0;
    if (has_match[i]) {
      if (r2l) {
        match_str[i] = substring(gen, ndr + 1, sub_dim[i], lane);
        init_left = al.isoa + sub_dim[i] + 1;
      } else {
        match_str[i] = substring(gen, nalg - sub_dim[i], sub_dim[i], lane);
        init_right = al.ieoa - sub_dim[i] - 1;
      }
    }
    has_ext_match[i] = has_match[i] && has_cut[i] && use_ext;
  }

  // every distance the decision below can ask for (ef_refine_intron.c:262-288): <= 2 + 4
  unsigned ed_prev[2], ed_pair[2][2];
  bool too_long = false;
  __syncthreads();                                                  // the pieces of the rows are in LDS
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ed_prev[i] = 0;
    if (variant1 && has_cut[i]) {
      const int la = stage_operand(L.a, est, cut_factor[i], L.ext_est, 0, true, lane);
      const int lb = stage_operand(L.b, gen, prev_match[i], L.ext_gen, 0, true, lane);
      __syncthreads();
      if (la < 0 || lb < 0) too_long = true;
      else ed_prev[i] = (unsigned)wave_edit_distance(L.a, la, L.b, lb, L.diag, lane);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ed_pair[i][j] = 0;
      const bool ext = has_ext_cut[i] && has_ext_match[j];
      if (ext || (has_cut[i] && has_match[j])) {
        const int la = stage_operand(L.a, est, cut_factor[i], L.ext_est, ext ? n_ext_est : 0, r2l, lane);
        const int lb = stage_operand(L.b, gen, match_str[j], L.ext_gen, ext ? n_ext_gen : 0, r2l, lane);
        __syncthreads();
        if (la < 0 || lb < 0) too_long = true;
        else ed_pair[i][j] = (unsigned)wave_edit_distance(L.a, la, L.b, lb, L.diag, lane);
      }
    }
  }
  if (too_long) return -1;

  bool stop = false;
  if (variant1) {
    unsigned error = 1000, edit_prev = 1000;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (!stop) {
          if (has_cut[i] && has_match[j]) {
            edit_prev = ed_prev[i];
            if (edit_prev <= 5) {
              if (has_ext_cut[i] && has_ext_match[j]) error = ed_pair[i][j] - edit_prev - (unsigned)ext_error;
              else error = ed_pair[i][j] - edit_prev;
            }
          }
          if (error <= 1) {
            if (r2l) { out_factor_left = naf + est_cut[i]; out_donor_right = ndr + sub_dim[j]; out_acc_left = nalg + gen_cut[i]; }
            else { out_factor_left = naf - est_cut[i]; out_donor_right = ndr - gen_cut[i]; out_acc_left = nalg - sub_dim[j]; }
            stop = true;
          }
        }
      }
    }
  } else {
    int error = 1000, edit = 1000;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (!stop) {
          if (has_ext_cut[i] && has_ext_match[j]) edit = (int)ed_pair[i][j] - ext_error;
          else if (has_cut[i] && has_match[j]) edit = (int)ed_pair[i][j];
          else edit = 1000;
          if (edit < error) {
            error = edit;
            if (r2l) { out_factor_left = naf + est_cut[i]; out_donor_right = ndr + sub_dim[j]; out_acc_left = nalg + gen_cut[i]; }
            else { out_factor_left = naf - est_cut[i]; out_donor_right = ndr - gen_cut[i]; out_acc_left = nalg - sub_dim[j]; }
          }
          if (error == 0) stop = true;
        }
      }
    }
  }
  return stop ? 1 : 0;
}

// The decision for one intron from its rows (`dim` bytes each, staged in LDS by the caller, who has synchronised behind
// the staging) and v[1..5] of its gap alignment in `q`; r arrives as PGPU_OK, not refined, path 0, the two factors of q.
__device__ __forceinline__ void refine_decide(RefineLds& L, const uint8_t* e_row, const uint8_t* g_row, const int dim,
                                              const pgpu_refine_query& q, const uint8_t* __restrict__ T, const uint32_t n,
                                              const uint8_t* __restrict__ ests, const int lane, pgpu_refine_result& r) {
  Rows al;
  al.e = e_row; al.g = g_row; al.dim = dim;
  al.glen = row_strlen(al.g, dim, lane); al.elen = row_strlen(al.e, dim, lane);
  al.isoa = q.intron_start_on_align; al.ieoa = q.intron_end_on_align;
  Seq est, gen;
  est.p = ests + q.est_off; est.len = (int)q.est_len;
  gen.p = T; gen.len = (int)n;
  const pgpu_factor d = q.donor, a = q.acceptor;
  // :55-64, :110, :123-125
  int dsl_gen = d.GEN_start;
  if (d.GEN_end - q.suffpref_length_on_gen + 1 >= dsl_gen) dsl_gen = d.GEN_end - q.suffpref_length_on_gen + 1;
  int dsl_est = d.EST_start;
  if (d.EST_end - q.suffpref_length_on_est + 1 >= dsl_est) dsl_est = d.EST_end - q.suffpref_length_on_est + 1;
  const int deleted_intron_dim = a.GEN_start - d.GEN_end - 1 - 2 * q.suffpref_length_for_intron;
  const int naf = dsl_est + q.factor_cut;
  const int ndr = dsl_gen + q.intron_start - 1;
  const int nalg = dsl_gen + q.intron_end + deleted_intron_dim + 1;
  const int dshift = ndr > d.GEN_end ? ndr - d.GEN_end : d.GEN_end - ndr;
  const int ashift = nalg > a.GEN_start ? nalg - a.GEN_start : a.GEN_start - nalg;
  if (naf == d.EST_start) {
    if (q.flags & PGPU_REFINE_FIRST_INTRON) { r.acceptor.EST_start = naf; r.acceptor.GEN_start = nalg; r.refined = 1; r.path = 0; }
    else r.path = 1;
  } else if (nalg - ndr < q.min_intron_length) {
    r.path = 2;
  } else if (dshift > 20 || ashift > 20) {
    r.path = 3;
  } else {
    int lc, lg, le, rc, rg, re;
    find_before_left(al, al.isoa - 1, 'G', 'T', lane, lc, lg, le);
    find_AG_after_right(al, al.ieoa + 1, lane, rc, rg, re);
    int fin_d = ndr, fin_a = nalg, fin_f = naf;
    bool accept = true;
    if (lg == 0 && rg == 0) {
      r.path = 4;
    } else {
      int settled = 0, sd = 0, sa = 0, sf = 0;
      int variant = 0;
      for (; variant < 4 && settled == 0; ++variant) {
        sd = sa = sf = 0;
        settled = shift_generic(L, est, gen, al, naf, ndr, nalg, (variant & 1) == 0, variant < 2, variant < 2 ? 'T' : 'C', lane,
                                sd, sa, sf);
      }
      if (settled < 0) {
        r.status = PGPU_ERANGE; accept = false;
      } else {
        if (settled == 1) r.path = 4 + variant;
        else {
          r.path = 9;
          sf = naf; sd = ndr; sa = nalg;
          const int el = substring(est, 0, est.len, lane).len;
          try_burset_after_match(est, gen, el, sf, sd, sa, d.EST_start, a.EST_end);
        }
        fin_d = sd; fin_a = sa; fin_f = sf;
        if (fin_a > a.GEN_end || fin_d < d.GEN_start) accept = false;
      }
    }
    if (accept) {
      r.donor.GEN_end = fin_d; r.acceptor.GEN_start = fin_a; r.acceptor.EST_start = fin_f; r.donor.EST_end = fin_f - 1;
      r.refined = 1;
    }
  }
}

}  // namespace
