"""What the compiler made of pgpu_tail_wide.hip and pgpu_small_wide.hip (no GPU needed: hipcc cross-compiles gfx950 here): the
checks of test_tail_resources.py and test_small_resources.py for the two kernels that answer the queries the narrow ones
refuse for a window -- exactly one kernel each with its dynamic programs inlined at 16 rows per lane, no scratch, no spilled
vector register, and the LDS of a workgroup, which is one wave, at the sum of the parts the head comment of each file
states.  The register and occupancy bounds are what the compiler reports for this build (tail_wide_kernel: 142 VGPRs, 3 waves
per SIMD; small_wide_kernel: 188 VGPRs, 2 waves per SIMD: DESIGN.md section 5r)."""
from resource_lib import usage as _usage


def test_tail_wide_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_tail_wide.hip", tmp_path)
    assert len(usage) == 1 and "tail_wide_kernel" in next(iter(usage)), sorted(usage)     # exactly one kernel
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        # the exons, the four row-minimum arrays of step 5, a job's result, the step bytes, the two reversed windows
        assert u["LDS Size"] == 64 * 16 + 4 * 129 * 4 + 48 + 64 + 1024 + 1200 == 5424, (name, u)
        assert u["VGPRs"] <= 142 and u["Occupancy"] >= 3, (name, u)


def test_small_wide_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_small_wide.hip", tmp_path)
    kernels = [n for n in usage if "small_wide_kernel" in n]
    assert len(kernels) == 1 and not [n for n in usage if "kernel" in n and n not in kernels], sorted(usage)
    u = usage[kernels[0]]
    assert u["ScratchSize"] == 0, u
    assert u["VGPRs Spill"] == 0, u
    # the list, the four row-minimum arrays of step 1, a job's result, the step bytes, the prefix piece
    assert u["LDS Size"] == 128 * 16 + 4 * 1025 * 4 + 48 + 128 + 64 == 18688, u
    assert u["VGPRs"] <= 188 and u["Occupancy"] >= 2, u
