/* The host side of tools/text_cost.py: what one thread of est-fact spends on the two text files of a chunk -- the
 * product's own ef_raw_text_from_records (pintron_amd/host/ef_records.c) over the records, and ef_write_single_est_info
 * (ef_io.c) per aligned EST -- into memory sinks, in CPU time of the calling thread.
 *   text_cost_host <genomic> <records.bin> <processed-ests.txt> <raw-multifasta-out.txt> <repeats>
 * The first three are the inputs, the fourth what the device wrote for the same records: both texts must equal the
 * device's.  Prints one line: "<raw ms> <pests ms>" per repeat.  Linked against pintron_amd/lib/libestfact.so. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../pintron_amd/host/estfact.h"

static char* slurp(const char* path, size_t* len) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "text_cost_host: cannot read %s\n", path); exit(2); }
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

static double cpu_ms(void) {
  struct timespec t;
  clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t);
  return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  size_t gl, rl, pl, wl;
  char* G = slurp(argv[1], &gl);
  char* rec = slurp(argv[2], &rl);
  char* pests = slurp(argv[3], &pl);
  char* want = slurp(argv[4], &wl);
  const int repeats = atoi(argv[5]);
  ef_seq gen;
  memset(&gen, 0, sizeof gen);
  gen.original_seq = G;
  /* the ESTs as est-fact holds them when it prints: header and sequence as C strings */
  size_t n = 0;
  for (size_t k = 0; k < pl; ++k) n += pests[k] == '\n';
  n /= 2;
  ef_seq* est = (ef_seq*)calloc(n ? n : 1, sizeof *est);
  char* copy = (char*)malloc(pl + 1);
  memcpy(copy, pests, pl + 1);
  char* p = copy;
  for (size_t k = 0; k < n; ++k) {
    char* nl = strchr(p, '\n'); *nl = '\0'; est[k].id = p + 1; p = nl + 1;
    nl = strchr(p, '\n'); *nl = '\0'; est[k].original_seq = p; p = nl + 1;
  }
  for (int r = 0; r < repeats; ++r) {
    ef_sink raw = { NULL, NULL, 0, 0 }, out = { NULL, NULL, 0, 0 };
    const double t0 = cpu_ms();
    if (ef_raw_text_from_records(&gen, rec, rl, pests, pl, &raw) != 0) { fprintf(stderr, "text_cost_host: inconsistent records\n"); return 1; }
    const double t1 = cpu_ms();
    for (size_t k = 0; k < n; ++k) ef_write_single_est_info(&out, &est[k]);
    const double t2 = cpu_ms();
    if (raw.len != wl || memcmp(raw.mem, want, wl) != 0 || out.len != pl || memcmp(out.mem, pests, pl) != 0) {
      fprintf(stderr, "text_cost_host: the host's text differs from the device's\n");
      return 1;
    }
    printf("%.4f %.4f\n", t1 - t0, t2 - t1);
    free(raw.mem); free(out.mem);
  }
  return 0;
}
