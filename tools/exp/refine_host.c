/* Host baseline of tools/refine_cost.py: refine_intron's decision from the gap alignment onward by the product's own
 * host code -- pintron_amd/host/ef_refine_intron.c, included here for its static routines (find_*, shift_generic,
 * try_burset_after_match) -- with the edit distances computed on the CPU (plain Levenshtein, two rows) instead of
 * asked from the device.  The part of ef_refine_intron() behind the alignment (:455-509) is repeated below with the
 * branch number the library reports.  One thread.
 *   gcc -O2 -fPIC -shared -o refine_host.so refine_host.c */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>

#include "../../pintron_amd/host/ef_refine_intron.c"

unsigned ef_genomic_epoch = 0;
int ef_prof_on = 0;
_Thread_local ef_prof_state ef_prof;
int ef_dp_many_ahead(ef_backend* be, const ef_dp_req* reqs, ef_dp_res* res, size_t n) { (void)be; (void)reqs; (void)res; (void)n; return -1; }

typedef struct { int32_t EST_start, EST_end, GEN_start, GEN_end; } factor;
typedef struct {
  uint64_t est_off; uint32_t est_len, flags; uint64_t rows_off; uint32_t dim;
  int32_t factor_cut, intron_start, intron_end, intron_start_on_align, intron_end_on_align;
  factor donor, acceptor;
  int32_t suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen, min_intron_length;
} refine_query;
typedef struct { int32_t status, refined, path, pad; factor donor, acceptor; } refine_result;

static int cpu_ed_many(void* self, const ef_dp_req* q, ef_dp_res* rs, size_t n) {
  (void)self;
  for (size_t k = 0; k < n; ++k) {
    uint32_t row[2][1100];
    const size_t la = q[k].la, lb = q[k].lb;
    if (lb >= 1100) return -1;
    for (size_t j = 0; j <= lb; ++j) row[0][j] = (uint32_t)j;
    for (size_t i = 1; i <= la; ++i) {
      uint32_t* cur = row[i & 1]; const uint32_t* prev = row[(i - 1) & 1];
      cur[0] = (uint32_t)i;
      for (size_t j = 1; j <= lb; ++j) {
        uint32_t v = prev[j - 1] + (q[k].a[i - 1] != q[k].b[j - 1]);
        if (prev[j] + 1 < v) v = prev[j] + 1;
        if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
        cur[j] = v;
      }
    }
    rs[k].v[0] = (int32_t)row[la & 1][lb];
  }
  return 0;
}

/* est: every EST NUL-terminated in `ests`; gen NUL-terminated; rows as the library takes them */
void refine_host_batch(const char* gen, const char* ests, const char* rows, const refine_query* q, size_t n, refine_result* out) {
  ef_backend be;
  memset(&be, 0, sizeof be);
  be.dp_many = cpu_ed_many;
  static char buf[2][8 + 1024 + 32];
  for (size_t k = 0; k < n; ++k) {
    const refine_query* x = &q[k];
    refine_result r;
    memset(&r, 0, sizeof r);
    r.donor = x->donor; r.acceptor = x->acceptor;
    if (x->dim > 1024) { r.status = -34; out[k] = r; continue; }
    memset(buf, 0, sizeof buf);                     /* the scans run a little past both ends of the rows */
    memcpy(buf[0] + 8, rows + x->rows_off, x->dim);
    memcpy(buf[1] + 8, rows + x->rows_off + x->dim, x->dim);
    const char* E = ests + x->est_off;
    gap_aln al;
    al.est_row = buf[0] + 8; al.gen_row = buf[1] + 8; al.dim = (int)x->dim;
    al.factor_cut = x->factor_cut; al.intron_start = x->intron_start; al.intron_end = x->intron_end;
    al.intron_start_on_align = x->intron_start_on_align; al.intron_end_on_align = x->intron_end_on_align;
    int dsl_gen = x->donor.GEN_start, dsl_est = x->donor.EST_start;
    if (x->donor.GEN_end - x->suffpref_length_on_gen + 1 >= dsl_gen) dsl_gen = x->donor.GEN_end - x->suffpref_length_on_gen + 1;
    if (x->donor.EST_end - x->suffpref_length_on_est + 1 >= dsl_est) dsl_est = x->donor.EST_end - x->suffpref_length_on_est + 1;
    const int deleted = x->acceptor.GEN_start - x->donor.GEN_end - 1 - 2 * x->suffpref_length_for_intron;
    al.new_acceptor_factor_left = dsl_est + al.factor_cut;
    al.new_donor_right_on_gen = dsl_gen + al.intron_start - 1;
    al.new_acceptor_left_on_gen = dsl_gen + al.intron_end + deleted + 1;
    if (al.new_acceptor_factor_left == x->donor.EST_start) {
      if (x->flags & 1u) { r.acceptor.EST_start = al.new_acceptor_factor_left; r.acceptor.GEN_start = al.new_acceptor_left_on_gen; r.refined = 1; }
      else r.path = 1;
    } else if (al.new_acceptor_left_on_gen - al.new_donor_right_on_gen < x->min_intron_length) {
      r.path = 2;
    } else if (abs(al.new_donor_right_on_gen - x->donor.GEN_end) > 20 || abs(al.new_acceptor_left_on_gen - x->acceptor.GEN_start) > 20) {
      r.path = 3;
    } else {
      int lc = 0, lg = 0, le2 = 0, rc = 0, rg = 0, re = 0;
      find_before_left(&al, al.intron_start_on_align - 1, &lc, &lg, &le2, "GT");
      find_AG_after_right(&al, al.intron_end_on_align + 1, &rc, &rg, &re);
      int fd = al.new_donor_right_on_gen, fa = al.new_acceptor_left_on_gen, ff = al.new_acceptor_factor_left, ok = 1;
      if (lg == 0 && rg == 0) r.path = 4;
      else {
        static const struct { bool r2l, v1; const char* pat; } variant[4] = { { true, true, "GT" }, { false, true, "GT" }, { true, false, "GC" }, { false, false, "GC" } };
        int sd = 0, sa = 0, sf = 0, v = 0;
        for (; v < 4; ++v) {
          sd = sa = sf = 0;
          if (shift_generic(E, gen, &al, variant[v].r2l, variant[v].v1, variant[v].pat, &sd, &sa, &sf, &be)) break;
        }
        r.path = 5 + v;
        if (v == 4) {
          sf = al.new_acceptor_factor_left; sd = al.new_donor_right_on_gen; sa = al.new_acceptor_left_on_gen;
          try_burset_after_match(E, gen, &sf, &sd, &sa, x->donor.EST_start, x->acceptor.EST_end);
        }
        fd = sd; fa = sa; ff = sf;
        if (fa > x->acceptor.GEN_end || fd < x->donor.GEN_start) ok = 0;
      }
      if (ok) { r.donor.GEN_end = fd; r.acceptor.GEN_start = fa; r.acceptor.EST_start = ff; r.donor.EST_end = ff - 1; r.refined = 1; }
    }
    out[k] = r;
  }
}
