/* TEST INFRASTRUCTURE (tests/): runs the host-side MEG construction of the est-fact program on
 * genomic.txt / ests.txt of the current directory with the CPU pairing ORACLE as the backend, and
 * writes megs-check.txt in the reference's megs.txt record format for EVERY entry of the EST
 * list (both strands).  With MEG_CHECK_FIRST_ATTEMPT=1 it writes megs-first.txt instead: for every
 * entry the graph of the FIRST attempt of build_meg (no retry with a longer factor), as
 *   "@@seq <prepared sequence>\n@@complex <0|1>\n@@stats <name=value ...>\n<meg_write text>@@edges\n<meg-edges text>@@end\n"
 * which is what the device's MEG stage returns per pattern (tests/test_gpu_pairings.py, tests/test_gpu_meg.py).
 * The @@stats line says what a builder with fixed arrays has to hold for this graph (tests/meg_lib.py derives
 * from it whether the device may, or must, flag the record PGPU_MEG_UNAVAILABLE):
 *   pairings=N                      vertices of build_vertex_set (source and sink not counted)
 *   build= simp= red= end=V,E,A,I   live vertices, edges, longest adjacency list, longest incidence list after
 *                                   ef_build_edge_set, ef_simplify_meg, the transitive reduction (= simp when it
 *                                   is switched off) and at the end
 *   created=C peak=P                ef_meg.diag_created and .diag_peak_list of ef_compact_short_edges
 *   clause=<name>                   what decided the too_complex verdict, recomputed here from tp, te, the
 *                                   frequency of the shortest pairing and the EST length: compaction
 *                                   (is_too_complex_for_compaction), early (fewer than 5 vertices or 4 edges),
 *                                   cmeg, edges (te > 5 tp), density (tp > 2 len / L), tp50, none
 * The product binary never links this file nor the oracle. */
#include <stdlib.h>
#include <string.h>

#include "../../pintron_amd/host/estfact.h"
#include "../../oracle/pairing_oracle.h"

static int oracle_pairings(void* self, const char* pattern, size_t m, unsigned L, double rate,
                           ef_triple** out, size_t* n) {
  long cap = 4096;
  int32_t* buf = (int32_t*)malloc(3 * cap * sizeof(int32_t));
  long cnt = orc_pairings((const orc_index*)self, pattern, m, L, rate, buf, cap, NULL);
  if (cnt > cap) {
    cap = cnt; buf = (int32_t*)realloc(buf, 3 * cap * sizeof(int32_t));
    cnt = orc_pairings((const orc_index*)self, pattern, m, L, rate, buf, cap, NULL);
  }
  *out = (ef_triple*)buf; *n = (size_t)cnt;
  return 0;
}

typedef struct { size_t v, e, adj, inc; } graph_counts;
static graph_counts count_graph(ef_meg* V) {
  graph_counts c = { 0, 0, 0, 0 };
  EF_MEG_FOR_POS(V, i, 0, V->n) {
    ef_iter it = efl_begin(V->v[i]);
    while (efi_has_next(&it)) {
      const ef_pairing* p = (const ef_pairing*)efi_next(&it);
      ++c.v; c.e += efl_size(p->adjs);
      if (efl_size(p->adjs) > c.adj) c.adj = efl_size(p->adjs);
      if (efl_size(p->incs) > c.inc) c.inc = efl_size(p->incs);
    }
  }
  return c;
}

/* the clause of is_too_complex (src/meg-simplification.c:89-139) that decides, from the numbers it looks at */
static const char* deciding_clause(ef_meg* V, const ef_config* cfg, bool* verdict) {
  int min_len = 0;
  size_t freq = 0, tp = 0, te = 0;
  const size_t est_len = V->n - 2;
  EF_MEG_FOR_POS(V, i, 0, V->n) {
    ef_iter it = efl_begin(V->v[i]);
    while (efi_has_next(&it)) {
      const ef_pairing* p = (const ef_pairing*)efi_next(&it);
      ++tp; te += efl_size(p->adjs);
      if (min_len == 0 || p->l < min_len) { min_len = p->l; freq = 1; }
      else if (p->l == min_len) ++freq;
    }
  }
  *verdict = true;
  if (tp < 5 || te < 4) { *verdict = false; return "early"; }
  if (cfg->max_pairings_in_MEG != 0 && tp > cfg->max_pairings_in_MEG && (double)freq > cfg->max_freq_shortest_pairing * (double)tp) return "cmeg";
  if (te > 5 * tp) return "edges";
  if (tp > (2 * est_len) / cfg->min_factor_len) return "density";
  if (tp > est_len / cfg->min_factor_len && tp >= 50) return "tp50";
  *verdict = false;
  return "none";
}

int main(int argc, char** argv) {
  ef_config cfg;
  if (ef_config_load(&cfg, argc, argv) != 0) return 2;
  ef_seq** gens; ef_seq** ests;
  if (ef_read_multifasta("genomic.txt", &gens) != 1) { fprintf(stderr, "genomic.txt: need exactly one sequence\n"); return 1; }
  ef_seq* gen = gens[0];
  ef_parse_genomic_header(gen);
  if (ef_ntails_removal(gen) != 0) return 1;
  const long n = ef_read_multifasta("ests.txt", &ests);
  if (n < 0) return 1;
  orc_index* ix = orc_index_create(gen->seq, strlen(gen->seq));
  if (getenv("MEG_CHECK_FIRST_ATTEMPT")) {         /* the genomic sequence as the index sees it */
    FILE* gp = fopen("genomic-prepared.txt", "w");
    fputs(gen->seq, gp);
    fclose(gp);
  }
  ef_backend be;
  memset(&be, 0, sizeof be);
  be.self = ix; be.pairings = oracle_pairings;
  ef_sink sink = { fopen("megs-check.txt", "w"), NULL, 0, 0 };
  ef_sink* f = &sink;
  for (long i = 0; i < n; ++i) {
    ef_seq* est = ests[i];
    ef_set_gb_identification(est);
    ef_set_strand_and_rc(est);
    ef_polyAT_substitution(est);
    ef_seq* both[2] = { est, NULL };
    if (!est->fixed_strand) { both[1] = ef_copy_and_reverse(est); ef_polyAT_substitution(both[1]); }
    for (int k = 0; k < 2 && both[k]; ++k) {
      if (getenv("MEG_CHECK_FIRST_ATTEMPT")) {
        static ef_sink first;
        if (!first.f) first.f = fopen("megs-first.txt", "w");
        ef_triple* tr = NULL; size_t ntr = 0;
        const size_t m = strlen(both[k]->seq);
        oracle_pairings(ix, both[k]->seq, m, cfg.min_factor_len, cfg.min_string_depth_rate, &tr, &ntr);
        ef_meg* V = ef_meg_from_pairings(tr, ntr, m);
        free(tr);
        if (V->diag_created != 0 || V->diag_peak_list != 0) { fprintf(stderr, "the diagnostic counters of a new graph are not zero\n"); return 3; }
        ef_build_edge_set(V, &cfg);
        const graph_counts c_build = count_graph(V);
        ef_simplify_meg(V, &cfg);
        const graph_counts c_simp = count_graph(V);
        if (cfg.trans_red) ef_transitive_reduction(V);
        const graph_counts c_red = count_graph(V);
        bool cx = ef_is_too_complex_for_compaction(V);
        const bool cx_before = cx;
        if (!cx && cfg.short_edge_comp) ef_compact_short_edges(V, &cfg);
        cx = cx || ef_is_too_complex(V, &cfg);
        const graph_counts c_end = count_graph(V);
        bool verdict;
        const char* clause = deciding_clause(V, &cfg, &verdict);
        if (cx_before) { clause = "compaction"; verdict = true; }
        if (verdict != cx) { fprintf(stderr, "the recomputed too_complex verdict differs from ef_is_too_complex\n"); return 3; }
        ef_sink_puts(&first, "@@seq "); ef_sink_puts(&first, both[k]->seq);
        ef_sink_puts(&first, cx ? "\n@@complex 1\n" : "\n@@complex 0\n");
        char st[400];
        snprintf(st, sizeof st, "@@stats pairings=%zu build=%zu,%zu,%zu,%zu simp=%zu,%zu,%zu,%zu red=%zu,%zu,%zu,%zu end=%zu,%zu,%zu,%zu "
                 "created=%zu peak=%zu clause=%s\n", ntr, c_build.v, c_build.e, c_build.adj, c_build.inc, c_simp.v, c_simp.e, c_simp.adj, c_simp.inc,
                 c_red.v, c_red.e, c_red.adj, c_red.inc, c_end.v, c_end.e, c_end.adj, c_end.inc, V->diag_created, V->diag_peak_list, clause);
        ef_sink_puts(&first, st);
        ef_meg_write(&first, V);
        ef_sink_puts(&first, "@@edges\n");
        ef_intronic_edges_write(&first, V);
        ef_sink_puts(&first, "@@end\n");
        ef_meg_free(V);
        continue;
      }
      size_t inc = 0;
      ef_meg* V = ef_build_meg(both[k], &be, &cfg, &inc);
      ef_sink_puts(f, "\n\n***********\n\n");
      ef_write_single_est_info(f, both[k]);
      ef_meg_write(f, V);
      ef_meg_free(V);
    }
  }
  fclose(sink.f);
  return 0;
}
