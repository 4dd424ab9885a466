// The rules of pgpu_index_small_chains that concern one query alone, beside the ones every chained entry checks
// (chained_queries_ok of pgpu_query_call.h, which calls this as the entry's own), and the rule on its parameters: plain
// code without a HIP call, in a header so that tests/hostcheck/small_call_check.cpp runs the very code of the entry under
// the sanitizers (as pgpu_tail.h).
#pragma once
#include "pgpu_tail.h"

// A small query is a tail query (pgpu_small_query is that type) and its input obeys the same rule: an EST of at least
// one byte, both sequences inside the buffer, every coordinate of every exon a byte of what it indexes.  Step 1 reads in
// front of the first exon and the steps read every exon on both sequences, so an end has to be a byte of its string.
// Order between the exons, or between an exon's two ends, is no rule here: the kernel refuses such a query (refused = 5),
// and its input has to be good all the same.  So is a query beyond PGPU_SMALL_MAX_EXONS (refused = 1).
PGPU_TAIL_HD static inline bool small_query_ok(const pgpu_small_query& x, const pgpu_factor* ex, size_t ests_len, size_t glen) {
  return tail_query_ok(x, ex, ests_len, glen);
}

// config->min_intron_length may be any value (the prefix search compares it raw, the search between two exons takes
// max(4, it)); only the reserved word is a rule
static inline bool small_params_ok(const pgpu_small_params* p) { return p != nullptr && p->reserved == 0; }
constexpr char SMALL_BAD_PARAMS[] = "bad small-chains parameters (reserved != 0)";
