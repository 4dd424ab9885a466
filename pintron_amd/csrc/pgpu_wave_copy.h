// The copy loop of the stages that print on the device (pgpu_text.hip, pgpu_side.hip): one routine, included by both.
// Device code; the caller's head comment says why no aligned load leaves the allocation it reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// dst[0 .. n) = src[0 .. n), by the whole wave; every argument is the same in all lanes
__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, uint32_t lane) {
  uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & 3u;
  if (head > n) head = n;
  if (lane < head) dst[lane] = src[lane];
  const uint32_t body = n - head, n_words = body >> 2, tail = body & 3u;
  uint32_t* __restrict__ const dw = (uint32_t*)(dst + head);
  const uint8_t* const s = src + head;
  const uint32_t sa = (uint32_t)(uintptr_t)s & 3u;
  const uint32_t* __restrict__ const sw = (const uint32_t*)(s - sa);
  if (sa == 0) {
    for (uint32_t i = lane; i < n_words; i += 64) dw[i] = sw[i];
  } else {
    for (uint32_t i = lane; i < n_words; i += 64) dw[i] = __builtin_amdgcn_alignbyte(sw[i + 1], sw[i], sa);
  }
  if (lane < tail) dst[head + 4 * n_words + lane] = src[head + 4 * n_words + lane];
}

}  // namespace
