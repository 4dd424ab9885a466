"""What the compiler made of pgpu_gaps.hip (no GPU needed: hipcc cross-compiles gfx950 here): the checks of
test_clean_resources.py for the kernel that chains the gaps of a factorization -- no scratch, no spilled vector registers,
and the LDS of a workgroup, which is one wave, pinned at its parts: the exons (64 x 16), their step bytes (64), the wave's
row-minimum region for the BORDERS mode (four arrays of 64 + 1 words) and the slot for that job's result (48)."""
from resource_lib import usage as _usage


def test_gaps_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_gaps.hip", tmp_path)
    assert len(usage) == 1 and "gaps_kernel" in next(iter(usage)), sorted(usage)          # exactly one kernel
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 64 * 16 + 64 + 4 * 65 * 4 + 48, (name, u)
        assert u["VGPRs"] <= 128 and u["Occupancy"] >= 4, (name, u)
