// How a device block is cut into parts: every part at a multiple of 256 bytes.  Plain host code without HIP, so that the
// layouts of the stage drivers (pgpu_fact.h, pgpu_final.h, pgpu_unit.h) build in tests/hostcheck under the sanitizers.
#pragma once
#include <stddef.h>

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// take(bytes): where the next part begins; an empty part still takes 256 bytes, so no two parts share an address.  A carver
// may begin behind a first part of the caller's: BlockCarver c{up256(first)}.
struct BlockCarver {
  size_t at = 0;
  size_t take(size_t bytes) { const size_t o = at; at += up256(bytes ? bytes : 1); return o; }
};
