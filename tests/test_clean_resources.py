"""What the compiler made of pgpu_clean.hip (no GPU needed: hipcc cross-compiles gfx950 here): the checks of
test_chain_resources.py for the kernel that chains a candidate's cleaning steps -- no scratch, no spilled vector
registers, and the LDS of one wave pinned at what the build reports: the traceback's direction window (8192) and path
(704), the exons (64 x 16) and their marks (64).  The direction words themselves live in HBM: DESIGN.md section 5g."""
from resource_lib import usage as _usage


def test_clean_kernel_has_no_stack_frame(tmp_path):
    usage = _usage("pgpu_clean.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "clean_kernel" in k}
    assert len(kernels) == 1, sorted(usage)
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 8192 + 704 + 64 * 16 + 64, (name, u)
        assert u["VGPRs"] <= 128 and u["Occupancy"] >= 4, (name, u)
