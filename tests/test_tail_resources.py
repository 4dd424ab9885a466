"""What the compiler made of pgpu_tail.hip (no GPU needed: hipcc cross-compiles gfx950 here): the checks of
test_gaps_resources.py for the kernel that chains the five steps behind the refinement loop -- exactly one kernel with its
three dynamic programs inlined, no scratch, no spilled vector registers, and the LDS of a workgroup, which is one wave,
pinned at its parts: the exons (64 x 16), the wave's row-minimum region for the BORDERS mode (four arrays of 128 + 1 words),
the slot for a job's result (48), the step bytes (64) and the two reversed windows of a lost prefix (256 + 304).  The
register and occupancy bounds are what the compiler reports for this build (93 VGPRs, 5 waves per SIMD: DESIGN.md section
5k), with the floor of gaps_kernel's test beneath them."""
from resource_lib import usage as _usage


def test_tail_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_tail.hip", tmp_path)
    assert len(usage) == 1 and "tail_kernel" in next(iter(usage)), sorted(usage)          # exactly one kernel
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 64 * 16 + 4 * 129 * 4 + 48 + 64 + 256 + 304 == 3760, (name, u)
        assert u["VGPRs"] <= 96 and u["Occupancy"] >= 5, (name, u)
