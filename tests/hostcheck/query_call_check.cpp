// The parts of pintron_amd/csrc/pgpu_query_call.h that make no HIP call, on the host alone: the rounding of the
// device offsets, the return code of a HIP error, and the range checks refine_introns and refine_chains share.
// Built with -fsanitize=address,undefined and run by tests/test_query_call_host.py; prints "ok" or the line that failed.
#include <limits.h>
#include <stdio.h>

#include "../../pintron_amd/csrc/pgpu_query_call.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
  EXPECT(up256(0) == 0 && up256(1) == 256 && up256(255) == 256 && up256(256) == 256 && up256(257) == 512);
  EXPECT(up256(0 + 64) == 256 && up256(192 + 64) == 256 && up256(193 + 64) == 512);      // the slack behind a string buffer
  EXPECT(up256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256);

  EXPECT(pgpu_code_of(hipErrorOutOfMemory) == PGPU_ENOMEM);
  EXPECT(pgpu_code_of(hipErrorInvalidValue) == PGPU_EDEVICE && pgpu_code_of(hipErrorIllegalAddress) == PGPU_EDEVICE &&
         pgpu_code_of(hipErrorLaunchFailure) == PGPU_EDEVICE && pgpu_code_of(hipErrorNoDevice) == PGPU_EDEVICE);

  EXPECT(coordinate_ok(-1, 0) && coordinate_ok(0, 0) && !coordinate_ok(1, 0) && !coordinate_ok(-2, 0));
  EXPECT(coordinate_ok(100, 100) && !coordinate_ok(101, 100) && !coordinate_ok(INT_MIN, 100));
  EXPECT(coordinate_ok(INT_MAX, (size_t)INT_MAX) && !coordinate_ok(INT_MAX, (size_t)INT_MAX - 1) && coordinate_ok(INT_MAX, (size_t)1 << 40));

  pgpu_factor f = { 0, 9, 100, 109 };
  EXPECT(factor_ok(f, 10, 110) && factor_ok(f, 9, 109) && !factor_ok(f, 8, 110) && !factor_ok(f, 10, 108));
  f.EST_start = -1; EXPECT(factor_ok(f, 10, 110));
  f.EST_start = -2; EXPECT(!factor_ok(f, 10, 110));
  f.EST_start = 11; EXPECT(!factor_ok(f, 10, 110));
  f.EST_start = 0; f.GEN_start = 111; EXPECT(!factor_ok(f, 10, 110));

  EXPECT(suffpref_ok(0, 0, 0) && suffpref_ok(30, 70, 30) && suffpref_ok(1 << 24, 1 << 24, 1 << 24));
  EXPECT(!suffpref_ok(-1, 70, 30) && !suffpref_ok(30, -1, 30) && !suffpref_ok(30, 70, -7));
  EXPECT(!suffpref_ok((1 << 24) + 1, 70, 30) && !suffpref_ok(30, (1 << 24) + 1, 30) && !suffpref_ok(30, 70, INT_MAX));

  if (!failures) printf("ok\n");
  return failures != 0;
}
