// getBursetFrequency as a table and its adaptor, for the units that instantiate the BORDERS mode of lev_wave_body
// (pgpu_wave_dp.h declares burset_adaptor and calls it): pgpu_dp_kernels.hip for the PGPU_DP_BORDERS jobs of a plan,
// pgpu_gaps.hip for the gaps of a factorization.  Include it behind pgpu_wave_dp.h.
#pragma once

#include "pgpu_wave_dp.h"

namespace {

// getBursetFrequency (src/refine-intron.c:376-556) as a table: index = donor[0],donor[1],
// acceptor[0],acceptor[1] at 2 bits each (A=0,C=1,G=2,T=3).
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

// getBursetFrequency_adaptor (src/refine-intron.c:362-374) over t with `avail` readable bytes
__device__ int burset_adaptor(const uint8_t* t, uint32_t avail, uint32_t cut1, uint32_t cut2) {
  if (cut2 < 2) return 0;
  if (cut1 + 1 >= avail || cut2 - 1 >= avail) return 0;   // a NUL terminates the C string
  const int c0 = acgt_code(t[cut1]), c1 = acgt_code(t[cut1 + 1]);
  const int c2 = acgt_code(t[cut2 - 2]), c3 = acgt_code(t[cut2 - 1]);
  if ((c0 | c1 | c2 | c3) < 0) return 0;
  return c_burset[(c0 << 6) | (c1 << 4) | (c2 << 2) | c3];
}

}  // namespace
