/* The host path pgpu_index_find would replace, for tools/find_cost.py: the strstr loop of the reference's
 * search_small_exon restated with memmem() over each query's window, one thread, advancing one byte behind
 * each hit.  Returns the number of occurrences; the positions go to out as far as cap allows. */
#define _GNU_SOURCE
#include <stddef.h>
#include <stdint.h>
#include <string.h>

size_t find_memmem_batch(const char* gen, size_t n, const char* pats, const uint64_t* pat_off, const uint32_t* pat_len,
                         const uint32_t* lo, const uint32_t* hi, size_t n_queries, uint32_t* out, size_t cap) {
  size_t total = 0;
  for (size_t q = 0; q < n_queries; ++q) {
    const size_t end = hi[q] < n ? hi[q] : n, len = pat_len[q];
    if (len == 0 || lo[q] > end || len > end - lo[q]) continue;
    const char* p = gen + lo[q];
    while ((p = memmem(p, (size_t)(gen + end - p), pats + pat_off[q], len))) {
      if (total < cap) out[total] = (uint32_t)(p - gen);
      ++total; ++p;
    }
  }
  return total;
}
