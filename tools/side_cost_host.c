/* The host side of tools/side_cost.py: what one thread of est-fact spends on the three side files of a chunk's settled
 * units -- the product's own code of ef_compute_est_fact (pintron_amd/host/ef_estfact.c:131-151) over the same MEG records:
 * per pattern a settled unit names, the record wrapped in an ef_meg (ef_meg_record_only), the separator,
 * ef_write_single_est_info and ef_meg_write into megs; for an aligned unit ef_intronic_edges_write behind its header line
 * into meg-edges, and the bytes megs has just got copied into processed-megs -- into memory sinks, in CPU time of the
 * calling thread.
 *   side_cost_host <recs.bin> <rec_first.bin> <units.bin> <headers.txt> <seqs.txt> <megs> <pmegs> <edges> <repeats>
 * units.bin: per settled unit four u32 (aligned, strand, fwd, rev); headers.txt: a line per settled unit; seqs.txt: a line
 * per pattern; the last three files are what the device wrote for the same units: all three texts must equal them.
 * Prints one line per repeat: "<ms>".  Linked against pintron_amd/lib/libestfact.so. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../pintron_amd/host/estfact.h"

static char* slurp(const char* path, size_t* len) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "side_cost_host: cannot read %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  char* p = (char*)malloc((size_t)n + 1);
  if (fread(p, 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  p[n] = '\0';
  *len = (size_t)n;
  return p;
}

/* the lines of a text as C strings, in place */
static char** lines_of(char* text, size_t len, size_t* n) {
  size_t count = 0;
  for (size_t k = 0; k < len; ++k) count += text[k] == '\n';
  char** out = (char**)malloc((count ? count : 1) * sizeof *out);
  char* p = text;
  for (size_t k = 0; k < count; ++k) { out[k] = p; char* nl = strchr(p, '\n'); *nl = '\0'; p = nl + 1; }
  *n = count;
  return out;
}

static double cpu_ms(void) {
  struct timespec t;
  clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t);
  return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}

static int same(const ef_sink* s, const char* want, size_t len) { return s->len == len && (len == 0 || memcmp(s->mem, want, len) == 0); }

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  size_t rl, fl, ul, hl, sl, wl[3], n_hdr, n_seq;
  char* recs = slurp(argv[1], &rl);
  const uint64_t* first = (const uint64_t*)slurp(argv[2], &fl);
  const uint32_t* units = (const uint32_t*)slurp(argv[3], &ul);
  char* hdr_text = slurp(argv[4], &hl);
  char* seq_text = slurp(argv[5], &sl);
  char* want[3];
  for (int k = 0; k < 3; ++k) want[k] = slurp(argv[6 + k], &wl[k]);
  const int repeats = atoi(argv[9]);
  char** headers = lines_of(hdr_text, hl, &n_hdr);
  char** seqs = lines_of(seq_text, sl, &n_seq);
  const size_t n = ul / 16;
  if (n != n_hdr || fl / 8 != n_seq + 1) { fprintf(stderr, "side_cost_host: the inputs do not fit each other\n"); return 2; }
  for (int r = 0; r < repeats; ++r) {
    ef_sink fmeg = { NULL, NULL, 0, 0 }, fpmeg = { NULL, NULL, 0, 0 }, fintronic = { NULL, NULL, 0, 0 };
    const double t0 = cpu_ms();
    for (size_t i = 0; i < n; ++i) {
      const uint32_t aligned = units[4 * i], strand = units[4 * i + 1];
      for (uint32_t s = 0; s <= strand; ++s) {
        const uint32_t x = units[4 * i + 2 + s];
        ef_seq est;
        memset(&est, 0, sizeof est);
        est.id = headers[i]; est.original_seq = seqs[x];
        ef_meg* V = ef_meg_record_only(recs + first[x], strlen(seqs[x]));
        ef_sink_puts(&fmeg, "\n\n***********\n\n");
        const size_t at = fmeg.len;
        ef_write_single_est_info(&fmeg, &est);
        ef_meg_write(&fmeg, V);
        if (aligned && s == strand) {
          ef_sink_puts(&fintronic, ">"); ef_sink_puts(&fintronic, est.id); ef_sink_puts(&fintronic, "\n");
          ef_intronic_edges_write(&fintronic, V);
          ef_sink_write(&fpmeg, fmeg.mem + at, fmeg.len - at);
        }
        ef_meg_free(V);
      }
    }
    const double t1 = cpu_ms();
    if (!same(&fmeg, want[0], wl[0]) || !same(&fpmeg, want[1], wl[1]) || !same(&fintronic, want[2], wl[2])) {
      fprintf(stderr, "side_cost_host: the host's text differs from the device's\n");
      return 1;
    }
    printf("%.4f\n", t1 - t0);
    free(fmeg.mem); free(fpmeg.mem); free(fintronic.mem);
  }
  return 0;
}
