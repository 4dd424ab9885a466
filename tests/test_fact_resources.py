"""What the compiler made of pgpu_fact.hip (no GPU needed: hipcc cross-compiles gfx950 here): the hand-off kernels of the
factorization driver, one thread per EST -- to clean, clean to gaps, gaps to refine, and the two passes of the gather --
and nothing else: no scratch (no per-thread array, no stack frame), no spilled register, no LDS.  The compiler reports
10 to 26 vector registers; the bound below leaves room before the test asks why."""
from resource_lib import usage as _usage

KERNELS = ("fact_to_clean_kernel", "fact_clean_to_gaps_kernel", "fact_gaps_to_refine_kernel", "fact_gather_kernelILb0",
           "fact_gather_kernelILb1")


def test_fact_kernels_have_no_stack_frame_and_no_lds(tmp_path):
    usage = _usage("pgpu_fact.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k in KERNELS:
        assert sum(k in name for name in usage) == 1, (k, sorted(usage))
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 0, (name, u)
        assert u["VGPRs"] <= 40 and u["Occupancy"] >= 8, (name, u)
