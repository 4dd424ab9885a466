"""What the compiler made of pgpu_cand.hip (no GPU needed: hipcc cross-compiles gfx950 here): the two instances of the
one-thread-per-record kernel, the count pass and the write pass, and nothing else; no scratch -- the fold keeps neither
the embedding nor the path in an array -- no spilled vector registers, no LDS.  The compiler reports 36 vector registers
for either instance; the bound below leaves it twelve more before the test asks why."""
from resource_lib import usage as _usage


def test_cand_kernels_have_no_stack_frame_and_no_lds(tmp_path):
    usage = _usage("pgpu_cand.hip", tmp_path)
    assert len(usage) == 2 and all("cand_kernel" in name for name in usage), sorted(usage)
    assert {name[name.index("cand_kernelILb") + len("cand_kernelILb")] for name in usage} == {"0", "1"}, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 0, (name, u)
        assert u["VGPRs"] <= 48 and u["Occupancy"] >= 8, (name, u)
