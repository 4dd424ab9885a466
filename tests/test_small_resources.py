"""What the compiler made of pgpu_small.hip (no GPU needed: hipcc cross-compiles gfx950 here): the checks of
test_tail_resources.py for the kernel that chains the last two routines of refine_EST_factorizations -- exactly one kernel
with its dynamic programs inlined (kband_band_sweep is a function of its own, as in clean_kernel), no scratch, no spilled
vector registers, and the LDS of a workgroup, which is one wave, pinned at its parts: the list (128 x 16), the wave's
row-minimum region for the BORDERS mode at four rows per lane (four arrays of 256 + 1 words), the slot for a job's result
(48), the step bytes (128) and the prefix piece (64).  The register and occupancy bounds are what the compiler reports for
this build (124 VGPRs, 4 waves per SIMD: DESIGN.md section 5m), with clean_kernel's bound above them."""
from resource_lib import usage as _usage


def test_small_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_small.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "small_kernel" in k}
    assert len(kernels) == 1 and all("small_kernel" in k or "kband_band_sweep" in k for k in usage), sorted(usage)
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 128 * 16 + 4 * 257 * 4 + 48 + 128 + 64 == 6400, (name, u)
        assert u["VGPRs"] <= 128 and u["Occupancy"] >= 4, (name, u)
